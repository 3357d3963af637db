"""bench.py's plain run and --dump-outputs.

A plain run (no --full) times its steps and prints the headline line without
the CPU baseline, the extras, the box probe or the oracle check; --steps sets
the number of timed steps.  --dump-outputs DIR writes what the last timed
step computed as float32 / float64 .npy files of at most 64 MB together: the
same sample for the same arguments (test_dump_sample_fixed, CPU), the same
values in two runs, and the oracle's values where the sample meets the
committed fingerprint of the same 48 sites (test_plain_run_dumps_outputs).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from util import GOLDEN, REPO

NPX = 2160 * 2560
LIMIT = 64 * 10 ** 6


def _dump_bytes(npx, n_sites, channels, only=None):
    plane_px, sites, site_px = bench.dump_sample(npx, n_sites, channels, only)
    per_file_header = 128
    return channels * (4 * 8 * len(plane_px) + 4 * len(sites) * len(site_px)
                       + (100000 + 65536) * 8 + 7 * per_file_header)


def test_dump_sample_fixed():
    a = bench.dump_sample(NPX, 3456, 1)
    b = bench.dump_sample(NPX, 3456, 1)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    plane_px, sites, site_px = a
    assert sites[0] == 0 and sites[-1] == 3455 and len(np.unique(sites)) == len(sites)
    for px in (plane_px, site_px):
        assert np.all(np.diff(px) > 0) and px[0] >= 0 and px[-1] < NPX
    assert _dump_bytes(NPX, 3456, 1) <= LIMIT
    assert _dump_bytes(NPX, 432, 4, only={0, 216, 431}) <= LIMIT
    assert _dump_bytes(NPX, 48, 4) <= LIMIT
    # a small job is kept whole
    plane_px, sites, site_px = bench.dump_sample(96 * 128, 6, 1)
    assert len(plane_px) == len(site_px) == 96 * 128 and sites.tolist() == list(range(6))


def _plain(tmp):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--sites",
                        "48", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp)],
                       cwd=REPO, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-4000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {n[:-4]: np.load(os.path.join(str(tmp), n))
                                  for n in sorted(os.listdir(str(tmp)))}


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_dumps_outputs(tmp_path):
    d, out = _plain(tmp_path / "a")
    # the headline alone: the timed steps, nothing measured or checked beside them
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1
    assert d["kernels"]["correct_hist"]["launches"] == 3
    assert d["ms_per_step"] > 0 and d["unit"] == "sites/s" and d["higher_is_better"] is True
    # value = sites / (ms_per_step / 1000), to the line's rounding (0.0005 ms, 0.05 sites/s)
    rate = 48 / (d["ms_per_step"] * 1e-3)
    assert abs(d["value"] - rate) <= rate * 0.0005 / d["ms_per_step"] + 0.1
    assert d["cpu_baseline"] is None and d["check_vs_oracle"] is None and d["check"] == {}
    assert "extras" not in d and "box" not in d
    # the files: float32 / float64, within the size limit
    assert sorted(out) == ["corrected", "histogram", "mean", "percentile_sums", "smoothed_mean",
                           "smoothed_std", "std"]
    assert out["corrected"].dtype == np.float32
    assert all(v.dtype == np.float64 for k, v in out.items() if k != "corrected")
    assert sum(os.path.getsize(str(tmp_path / "a" / n)) for n in os.listdir(str(tmp_path / "a"))) \
        <= LIMIT
    # against the oracle fingerprint of the same 48 sites, where the samples meet
    plane_px, sites, site_px = bench.dump_sample(NPX, 48, 1)
    assert out["mean"].shape == plane_px.shape and out["corrected"].shape == (len(sites),
                                                                             len(site_px))
    with np.load(os.path.join(GOLDEN, bench.fingerprint_name(2160, 2560, 48, bench.SEED, 0,
                                                             "synthetic"))) as z:
        fp = {k: z[k] for k in z.files}
    import hashlib
    assert hashlib.sha256(out["percentile_sums"].tobytes()).hexdigest() == \
        str(fp["pct_sums_sha256"])
    assert hashlib.sha256(out["histogram"].astype(np.uint64).tobytes()).hexdigest() == \
        str(fp["hist_sha256"])
    _, i_got, i_fp = np.intersect1d(plane_px, fp["stat_px"], return_indices=True)
    assert len(i_got) > 100
    for name, key in (("mean", "mean_samples"), ("std", "std_samples"),
                      ("smoothed_mean", "smean_samples"), ("smoothed_std", "sstd_samples")):
        got, want = out[name][i_got], fp[key][i_fp]
        assert np.all(np.abs(got - want) <= 1e-9 + 1e-6 * np.abs(want)), name
    _, j_got, j_fp = np.intersect1d(site_px, fp["corr_px"], return_indices=True)
    assert len(j_got) > 100
    met = 0
    for k, s in enumerate(fp["corr_sites"].tolist()):
        if s in sites.tolist():
            got = out["corrected"][sites.tolist().index(s)][j_got].astype(np.int64)
            want = fp["corr_samples"][k][j_fp].astype(np.int64)
            assert np.abs(got - want).max() <= 1, s  # +-1 DN, a wrap flip counts as 65535
            met += 1
    assert met >= 2  # the first and the last site are always sampled
    # the same arguments, the same inputs, the same outputs
    d2, out2 = _plain(tmp_path / "b")
    assert d2["steps"] == 3
    for name in out:
        assert np.array_equal(out[name], out2[name]), name
