"""CPU: the inputs of test_gpu_fix_overflow.py do what that file needs them
to -- more flagged pixels (or groups) than the fixup list holds, most of them
wrong if left unrefined -- from the oracle's f64 arithmetic alone
(tests/overflow_cases.py).  Conditions on the inputs, not measurements."""
import os
import re

import numpy as np
import pytest

import overflow_cases as oc
from util import REPO


def test_capacity_rule():
    assert oc.fix_capacity(5, 512 * 512) == 1 << 20
    assert oc.fix_capacity(2, 2160 * 2560) == 1 << 20
    assert oc.fix_capacity(3456, 2160 * 2560) == 3456 * 2160 * 2560 // 1024
    assert oc.fix_capacity(1 << 23, 1 << 22) == 1 << 30
    text = open(os.path.join(REPO, "tmlibrary_amd", "csrc", "abi_apply.hip")).read()
    assert "(int64_t)1 << 20, n_sites * c->npx / 1024" in text  # the rule restated above
    kern = open(os.path.join(REPO, "tmlibrary_amd", "csrc", "common.h")).read()
    k = dict(re.findall(r"constexpr double (kRefineK[12]) = ([0-9.e-]+);", kern))
    assert (float(k["kRefineK1"]), float(k["kRefineK2"])) == (oc.K1, oc.K2)


@pytest.mark.parametrize("name,clip", [("log", None), ("log", (1000, 60000)), ("nolog", None),
                                       ("nolog", (1000, 60000)), ("scalar", None), ("u8", None)])
def test_plain_cases_overflow(name, clip):
    case = {"log": oc.plain_log, "nolog": oc.plain_nolog, "u8": oc.plain_u8,
            "scalar": lambda: oc.plain_log((511, 513))}[name]()
    r = oc.check_pixel_overflow(case, clip)
    print(name, clip, r)
    if name == "scalar":
        assert case.npx % 8 == 7
    if name == "nolog":
        assert np.abs(case.f64()[case.flagged()]).min() > 2.0 ** 25


def test_full_size_case_overflows_by_groups():
    case = oc.full_size()
    r = oc.check_group_overflow(case)
    print(r)
    bad, fl = case.bad_if_unrefined(), case.flagged()
    for i in range(case.n):
        assert 2 * np.count_nonzero(bad[i]) >= np.count_nonzero(fl[i]) > 0


@pytest.mark.parametrize("bounds", [(100, 3000), (0, 65535)])
def test_chain_case_overflows_inside_the_windows(bounds):
    r, wins = oc.check_chain_overflow(oc.full_size(), bounds)
    print(bounds, r)
    assert int(wins[1]["src_r0"]) != int(wins[1]["dst_r0"])  # a shifted site


def test_stack_case_overflows_inside_the_windows():
    print(oc.check_stack_overflow(oc.plain_log()))
    site, slot, _ = oc.stack_layout()
    pairs = set(zip(site.tolist(), slot.tolist()))
    assert len(pairs) == 5 and (1, 1) not in pairs


def test_lds_set_case_fills_every_unit():
    case = oc.lds_set()
    groups = int(np.count_nonzero(case.flagged_groups()))
    assert groups == case.n * (case.npx // 8 - 1)  # every group but the large-std one
    assert groups < oc.fix_capacity(case.n, case.npx) // 8  # far under the list's capacity
    assert oc.min_unit_groups(case) > oc.FIX_SH
    bad = case.bad_if_unrefined()
    for i in range(case.n):
        assert 2 * np.count_nonzero(bad[i]) >= np.count_nonzero(case.flagged()[i])
    kern = open(os.path.join(REPO, "tmlibrary_amd", "csrc", "fused_kernels.hip")).read()
    assert "constexpr int kFixSh = %d;" % oc.FIX_SH in kern


def test_object_table_constants_match_the_header():
    from tmlibrary_amd import hip
    text = open(os.path.join(REPO, "include", "tmhip.h")).read()
    for name in ("OBJECT_SLOTS", "OBJECT_PROBE"):
        m = re.search(r"#define TMH_%s (\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(hip, name)
