"""Writes tests/golden/jpeg_decoded.npz: what libjpeg-turbo (through Pillow)
decodes from every out_* file of jpeg_tiles.npz (dec_<name>), ten more seeded
ragged tiles (in_/q_/file_/dec_extra<i>) coded and decoded by Pillow, and four
files Pillow writes that the decoder must report as unsupported (bad_<name>:
progressive, RGB, optimised Huffman tables, 257 pixels wide).
Data only; run from tests/ with Pillow installed:

    python golden/make_jpeg_decode_goldens.py
"""
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import jpeg_decode_literal as jd  # noqa: E402
import jpeg_literal as jl  # noqa: E402


def decoded(data):
    return np.array(Image.open(io.BytesIO(data)))


def main():
    out = {"pillow_version": np.array(PIL.__version__),
           "libjpeg_version": np.array("libjpeg-turbo %s (libjpeg API %s)" % (
               features.version("libjpeg_turbo"), features.version("jpg")))}
    for name, _, _, data in jl.load_goldens(os.path.join(HERE, "jpeg_tiles.npz")):
        out["dec_" + name] = decoded(data)
    rng = np.random.default_rng(14)
    for i, (kind, q) in enumerate(jd.EXTRA_CASES):
        h, w = (int(v) for v in rng.integers(1, 257, 2))
        if i % 3 == 0:
            h, w = min(h, 40), min(w, 40)
        a = jl.case_array(kind, (h, w), seed=1400 + i)
        buf = io.BytesIO()
        Image.fromarray(a, "L").save(buf, "JPEG", quality=q)
        n = "extra%d" % i
        out["in_" + n], out["q_" + n] = a, np.array(q)
        out["file_" + n] = np.frombuffer(buf.getvalue(), np.uint8)
        out["dec_" + n] = decoded(buf.getvalue())
    small = jl.case_array("cells", (40, 24), seed=7)
    for name, image, options in [
            ("progressive", Image.fromarray(small, "L"), dict(progressive=True)),
            ("rgb", Image.fromarray(np.stack([small] * 3, axis=-1), "RGB"), {}),
            ("optimised", Image.fromarray(small, "L"), dict(optimize=True)),
            ("wide257", Image.fromarray(jl.case_array("cells", (8, 257), seed=7), "L"), {})]:
        buf = io.BytesIO()
        image.save(buf, "JPEG", quality=95, **options)
        out["bad_" + name] = np.frombuffer(buf.getvalue(), np.uint8)
    path = os.path.join(HERE, "jpeg_decoded.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
