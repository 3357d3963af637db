"""Writes tests/golden/jpeg_tiles.npz: for the fixed case list of
tests/jpeg_literal.py (GOLDEN_CASES) the input array, the quality and the
bytes Pillow's bundled libjpeg-turbo writes for it
(``Image.fromarray(a, 'L').save(buf, 'JPEG', quality=q)``), plus the Pillow and
libjpeg versions.  Needs Pillow; the tests only read the file.

    python tests/golden/make_jpeg_goldens.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_literal as jl  # noqa: E402


def pillow_bytes(a, quality):
    buf = io.BytesIO()
    Image.fromarray(a, "L").save(buf, "JPEG", quality=quality)
    return buf.getvalue()


def main():
    out = {"pillow_version": np.array(PIL.__version__),
           "libjpeg_version": np.array(str(features.version("jpg"))),
           "libjpeg_turbo": np.array(bool(features.check_feature("libjpeg_turbo")))}
    for name, kind, shape, quality in jl.GOLDEN_CASES:
        a = jl.case_array(kind, shape)
        out["in_" + name] = a
        out["q_" + name] = np.array(quality)
        out["out_" + name] = np.frombuffer(pillow_bytes(a, quality), dtype=np.uint8)
    path = os.path.join(HERE, "jpeg_tiles.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; Pillow", PIL.__version__, "libjpeg",
          features.version("jpg"))


if __name__ == "__main__":
    main()
