"""hip.DeviceBuffer on the device, and a Pyramid that holds its levels in them."""
import numpy as np
import pytest

import pyramid_literal as lit
from tmlibrary_amd import hip
from tmlibrary_amd.image import tiles_to_array

pytestmark = pytest.mark.gpu
T = 256


def test_round_trip_at_offsets_0_and_256():
    a = np.random.default_rng(7).integers(0, 256, 1024, dtype=np.uint8)
    with hip.DeviceBuffer(1024) as buf:
        assert buf.ptr.value and buf.nbytes == 1024
        buf.put(a)
        assert np.array_equal(buf.get(1024, np.uint8), a)
        buf.put(a[:256][::-1], offset=256)
        assert np.array_equal(buf.get(256, np.uint8, offset=256), a[:256][::-1])
        tail = np.concatenate([a[:256][::-1], a[512:]])
        assert np.array_equal(buf.get((3, 64), np.uint32, offset=256),
                              tail.view(np.uint32).reshape(3, 64))
        assert np.array_equal(buf.get(256, np.uint8), a[:256])
    assert buf.ptr.value is None


def test_zero_bytes_is_a_null_pointer():
    with hip.DeviceBuffer(0) as buf:
        assert buf.ptr.value is None and buf.nbytes == 0


def test_pyramid_levels_live_in_device_buffers():
    """The smallest layer of pyramid_literal.py (2 x 4 base tiles; none of its
    layers has 3 x 3)."""
    from tmlibrary_amd.workflow.pyramid import build_pyramid
    g = lit.make_layer("tile_aligned")
    sites = lit.random_sites(g)
    want, _ = lit.literal_base_level(g, sites)
    with build_pyramid(g, sites) as pyr:
        z = pyr.depth - 1
        rows, cols = pyr.dimensions[z]
        assert (rows, cols) == want.shape[:2] == (2, 4)
        assert all(isinstance(b, hip.DeviceBuffer) for b in pyr._levels)
        assert pyr._levels[z].nbytes == rows * cols * T * T
        assert pyr.device_level(z)[0].value == pyr._levels[z].ptr.value
        assert np.array_equal(pyr.level(z), tiles_to_array(want, T, T))
        for y in range(rows):
            for x in range(cols):
                assert np.array_equal(pyr.tile(z, y, x).array, want[y, x]), (y, x)
        levels = list(pyr._levels)
    assert all(b.ptr.value is None for b in levels)
    with pytest.raises(ValueError, match="the pyramid is closed"):
        pyr._check(0)
