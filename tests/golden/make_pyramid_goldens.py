#!/usr/bin/env python3
"""Generate tests/golden/pyramid_*.{npz,json} from the REFERENCE itself.

Runs only where /root/reference exists.  Two sources:

* tmlib/image.py, imported with make_goldens.py's shims: ``Image.extract /
  insert / merge / join / pad_with_background`` and ``PyramidTile``'s checks;
* tmlib/models/channel.py, NOT imported (it pulls in the ORM): the five pure
  ``ChannelLayer`` methods are taken out of the file's syntax tree, compiled on
  their own and run against a stub ``self``.

Only inputs and results are written (data); no reference text is stored.

    python tests/golden/make_pyramid_goldens.py
"""
from __future__ import annotations

import ast
import itertools
import json
import logging
import os
import sys
import types

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens  # noqa: E402  (load_reference and its shims)

REF = make_goldens.REF
PURE = ("_calc_tile_indices_and_offsets", "_calc_tile_indices", "_get_image_sizes",
        "calc_coordinates_of_next_higher_level", "extract_tile_from_image")

POSITIONS = (0, 255, 256, 257, 500)
LENGTHS = (256, 300, 2160)
DISPLACEMENTS = (0, 7)
LAYER_SIZES = ((600, 1260), (1100, 1760), (256, 256), (257, 1), (4320, 7680), (70000, 110000))
LEVEL_DIMENSIONS = [(1, 1), (2, 3), (3, 5)]
TILE_OFFSETS = ((0, 0), (-44, -164), (44, 164), (-255, 100), (100, -1), (299, 419), (0, 164))


def load_channel_layer(image_mod):
    """The five pure methods of ChannelLayer as functions of a stub ``self``."""
    path = os.path.join(REF, "tmlib", "models", "channel.py")
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "ChannelLayer"][0]
    funcs = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in PURE]
    assert sorted(f.name for f in funcs) == sorted(PURE)
    for f in funcs:
        f.decorator_list = []
    ns = {"np": np, "itertools": itertools, "xrange": range,
          "logger": logging.getLogger("reference"), "PyramidTile": image_mod.PyramidTile}
    exec(compile(ast.Module(body=funcs, type_ignores=[]), path, "exec"), ns)

    class Layer(object):
        tile_size = 256
        dimensions = LEVEL_DIMENSIONS
        channel = types.SimpleNamespace(experiment=types.SimpleNamespace(zoom_factor=2))

    for name in PURE:
        setattr(Layer, name, ns[name])
    return Layer()


def error_of(fn):
    try:
        fn()
    except Exception as e:  # the type and message are the golden
        return [type(e).__name__, str(e)]
    return None


def main():
    metadata, image, _ = make_goldens.load_reference()
    layer = load_channel_layer(image)
    rng = np.random.default_rng(20240607)
    geo = {"positions": POSITIONS, "lengths": LENGTHS, "displacements": DISPLACEMENTS,
           "indices_and_offsets": [], "indices": [], "image_sizes": [], "next_higher": []}
    for p, n, d in itertools.product(POSITIONS, LENGTHS, DISPLACEMENTS):
        r = layer._calc_tile_indices_and_offsets(p, n, d)
        geo["indices_and_offsets"].append({"args": [p, n, d], "indices": list(r["indices"]),
                                           "offsets": list(r["offsets"])})
        geo["indices"].append({"args": [p, n, d], "indices": list(layer._calc_tile_indices(p, n, d))})
    for h, w in LAYER_SIZES:
        geo["image_sizes"].append({"args": [h, w],
                                   "sizes": [list(s) for s in layer._get_image_sizes(h, w)]})
    geo["level_dimensions"] = [list(d) for d in LEVEL_DIMENSIONS]
    for z in range(len(LEVEL_DIMENSIONS) - 1):
        for y, x in itertools.product(range(LEVEL_DIMENSIONS[z][0]), range(LEVEL_DIMENSIONS[z][1])):
            c = layer.calc_coordinates_of_next_higher_level(z, y, x)
            geo["next_higher"].append({"args": [z, y, x], "coordinates": [list(t) for t in c]})

    arrays = {}
    site = rng.integers(0, 256, (300, 420), dtype=np.uint8)
    arrays["site"] = site
    arrays["tile_offsets"] = np.array(TILE_OFFSETS, dtype=np.int64)
    for k, (yo, xo) in enumerate(TILE_OFFSETS):
        t = layer.extract_tile_from_image(image.Image(site), yo, xo)
        assert isinstance(t, image.PyramidTile)
        arrays["tile_%d" % k] = t.array

    # Image methods
    a = rng.integers(0, 256, (40, 50), dtype=np.uint8)
    b = rng.integers(0, 256, (40, 50), dtype=np.uint8)
    small = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    arrays.update(img_a=a, img_b=b, img_small=small)
    extracts = ((0, 10, 0, 10), (5, 7, 9, 11), (35, 10, 45, 10), (39, 1, 49, 1), (0, 40, 0, 50))
    arrays["extract_args"] = np.array(extracts, dtype=np.int64)
    for k, e in enumerate(extracts):
        arrays["extract_%d" % k] = image.Image(a).extract(*e).array.copy()
    arrays["insert_copy"] = image.Image(a).insert(image.Image(small), 3, 4, inplace=False).array
    ins = image.Image(a.copy())
    assert ins.insert(image.Image(small), 33, 41) is ins
    arrays["insert_inplace"] = ins.array
    arrays["merge_y"] = image.Image(a).merge(image.Image(b), "y", 13, inplace=False).array
    arrays["merge_x"] = image.Image(a).merge(image.Image(b), "x", 21, inplace=False).array
    arrays["join_y"] = image.Image(a).join(image.Image(b), "y").array
    arrays["join_x"] = image.Image(a).join(image.Image(b), "x").array
    for side in ("top", "bottom", "left", "right"):
        arrays["pad_" + side] = image.Image(small).pad_with_background(3, side).array
    arrays["background"] = image.PyramidTile.create_as_background().array

    u8 = np.zeros((4, 4), dtype=np.uint8)
    errors = {
        "insert_too_low": error_of(lambda: image.Image(a).insert(image.Image(small), 34, 0)),
        "insert_too_right": error_of(lambda: image.Image(a).insert(image.Image(small), 0, 42)),
        "merge_axis": error_of(lambda: image.Image(a).merge(image.Image(b), "z", 0)),
        "join_axis": error_of(lambda: image.Image(a).join(image.Image(b), "z")),
        "pad_side": error_of(lambda: image.Image(a).pad_with_background(1, "front")),
        "tile_uint16": error_of(lambda: image.PyramidTile(np.zeros((4, 4), dtype=np.uint16))),
        "tile_not_array": error_of(lambda: image.PyramidTile([[0]])),
        "tile_1d": error_of(lambda: image.PyramidTile(np.zeros(4, dtype=np.uint8))),
        "tile_too_high": error_of(lambda: image.PyramidTile(np.zeros((257, 4), dtype=np.uint8))),
        "tile_too_wide": error_of(lambda: image.PyramidTile(np.zeros((4, 257), dtype=np.uint8))),
        "tile_empty": error_of(lambda: image.PyramidTile(np.zeros((0, 4), dtype=np.uint8))),
        "tile_256": error_of(lambda: image.PyramidTile(np.zeros((256, 256), dtype=np.uint8))),
        "tile_metadata": error_of(lambda: image.PyramidTile(u8, metadata.ImageMetadata())),
        "tile_metadata_ok": error_of(
            lambda: image.PyramidTile(u8, metadata.PyramidTileMetadata(1, 2, 3, 4))),
        "background_noise_no_mu": error_of(
            lambda: image.PyramidTile.create_as_background(add_noise=True)),
        "background_noise_no_sigma": error_of(
            lambda: image.PyramidTile.create_as_background(add_noise=True, mu=3)),
        "background_noise": error_of(
            lambda: image.PyramidTile.create_as_background(add_noise=True, mu=3, sigma=1)),
    }
    geo["errors"] = errors
    with open(os.path.join(HERE, "pyramid_geometry.json"), "w") as f:
        json.dump(geo, f, indent=1, sort_keys=True)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "pyramid_image.npz"), **arrays)
    print("wrote pyramid_geometry.json, pyramid_image.npz (%d arrays, %d error cases)"
          % (len(arrays), len(errors)))


if __name__ == "__main__":
    main()
