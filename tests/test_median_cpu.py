"""Median-distance rejection: the rule itself (tests/median_ref.py, the restatement the GPU tests compare the device with) on hand-made
arrays — the lower median at n = 0 .. 3, ties, a median of 0, a threshold that rounds to +inf, a factor below 1, pairs that are no
candidates — and its relation to trimming at keep 0.5."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from icp_checks import trim_rule      # noqa: E402
from median_ref import median_rule, pick_factor, threshold      # noqa: E402


def pairs_of(d):
    """PF / PM whose geo is exactly d^2 for small integers d: the fixed points at the origin's side, the moving ones d along x."""
    d = np.asarray(d, np.float32)
    PF = np.zeros((d.size, 4), np.float32)
    PF[:, 2] = 1000.0
    PM = PF.copy()
    PM[:, 0] = d
    return PF, PM


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


def test_no_candidate():
    PF, PM = pairs_of([])
    acc, words = median_rule(PF, PM, np.zeros(0, np.float32), 2.0)
    assert acc.size == 0 and words.tolist() == [0, 0, 0, 0]
    PF, PM = pairs_of([1, 2, 3])
    acc, words = median_rule(PF, PM, np.zeros(3, np.float32), 2.0)
    assert not acc.any() and words.tolist() == [0, 0, 0, 0]


def test_lower_median_of_one_two_three():
    ones = lambda n: np.ones(n, np.float32)
    for d, t_med in (([3], 9.0), ([3, 1], 1.0), ([3, 1, 2], 4.0), ([4, 1, 2, 3], 4.0)):
        PF, PM = pairs_of(d)
        acc, words = median_rule(PF, PM, ones(len(d)), 1.0)
        assert words[0] == f32bits(t_med) and words[1] == len(d) and words[2] == f32bits(t_med), (d, words)
        assert acc.tolist() == [x * x <= t_med for x in d] and words[3] == np.count_nonzero(acc)


def test_ties_at_the_median_are_kept():
    PF, PM = pairs_of([1, 2, 2, 2, 2, 5, 6])
    acc, words = median_rule(PF, PM, np.ones(7, np.float32), 1.0)
    assert words.tolist() == [f32bits(4.0), 7, f32bits(4.0), 5]           # K = 4, and every pair at t_med is accepted
    assert acc.tolist() == [True] * 5 + [False] * 2


def test_median_of_zero():
    PF, PM = pairs_of([0, 0, 0, 1, 2])
    acc, words = median_rule(PF, PM, np.ones(5, np.float32), 3.0)
    assert words.tolist() == [0, 5, 0, 3] and acc.tolist() == [True, True, True, False, False]


def test_threshold_that_rounds_to_inf_accepts_every_candidate():
    PF, PM = pairs_of([1, 2, 3, 400])
    W0 = np.array([1, 1, 0, 1], np.float32)
    acc, words = median_rule(PF, PM, W0, 1e20)
    assert words.tolist() == [f32bits(4.0), 3, 0x7F800000, 3]
    assert acc.tolist() == [True, True, False, True]
    assert threshold(1e20, 1.0).view(np.uint32) == 0x7F800000 and np.isfinite(threshold(1e19, 1.0))      # (1e40 against 1e38)


def test_factor_below_one():
    PF, PM = pairs_of([1, 2, 3, 4, 5])
    acc, words = median_rule(PF, PM, np.ones(5, np.float32), 0.5)
    assert words.tolist() == [f32bits(9.0), 5, f32bits(2.25), 1] and acc.tolist() == [True, False, False, False, False]
    assert words[3] < (5 + 1) // 2


def test_the_product_is_taken_in_double_and_rounded_once():
    f, t = np.float32(1.1), np.float32(3.3)
    want = np.float32((np.float64(f) * np.float64(f)) * np.float64(t))
    assert threshold(1.1, t).view(np.uint32) == want.view(np.uint32)
    assert want.view(np.uint32) != ((f * f) * t).view(np.uint32) or want.view(np.uint32) != (f * (f * t)).view(np.uint32)


def test_no_candidates_are_left_out():
    """A weight of 0 and a geo that is NaN or inf make no candidate: they neither count nor move the median, and are not accepted."""
    PF, PM = pairs_of([1, 2, 3, 4, 5, 6, 7])
    PM[4, 0] = np.nan
    PM[5, 1] = np.inf
    W0 = np.array([1, 1, 1, 0, 1, 1, 1], np.float32)
    acc, words = median_rule(PF, PM, W0, 1.0)
    assert words.tolist() == [f32bits(4.0), 4, f32bits(4.0), 2]           # candidates 1, 2, 3, 7: K = 2
    assert acc.tolist() == [True, True, False, False, False, False, False]
    acc, words = median_rule(PF, PM, np.where(W0 != 0, np.float32(-0.25), 0).astype(np.float32), 1.0)      # (any weight != 0 counts)
    assert words[1] == 4


def test_factor_one_is_trimming_at_half():
    rng = np.random.default_rng(0x3ED1A)
    for n in (1, 2, 7, 64, 1001):
        PF = rng.normal(0, 50, (n, 4)).astype(np.float32)
        PM = (PF + rng.normal(0, 3, (n, 4))).astype(np.float32)
        PM[: n // 8] = PM[0]                                              # (ties)
        PF[: n // 8] = PF[0]
        W0 = (rng.random(n) < 0.9).astype(np.float32)
        am, wm = median_rule(PF, PM, W0, 1.0)
        at, wt = trim_rule(PF, PM, W0, 0.5)
        assert np.array_equal(am, at), n
        if wm[1]:
            assert wm[0] == wt[0] and wm[1] == wt[1] and wm[3] == wt[3] and wm[2] == wm[0] and wt[2] == (wm[1] + 1) // 2, (wm, wt)


def test_pick_factor_makes_the_rule_bite():
    rng = np.random.default_rng(0x3ED1B)
    for n in (20, 2500, 16384):
        PF = rng.normal(0, 50, (n, 4)).astype(np.float32)
        PM = (PF + rng.normal(0, 3, (n, 4))).astype(np.float32)
        W0 = np.ones(n, np.float32)
        acc, words = median_rule(PF, PM, W0, 1.0)
        from icp_checks import geo_of
        f = pick_factor(geo_of(PF, PM), 0.15)
        assert f > 1.0
        acc, words = median_rule(PF, PM, W0, f)
        assert 0 < words[3] < n and abs((n - int(words[3])) / n - 0.15) < 0.06, (n, words)


# ---- the interface that needs no device: the command lines and the keyword

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_register_command_line_has_the_option():
    import inspect
    import subprocess
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--median-factor" in r.stdout
    for bad in ("0", "-1", "nan", "inf"):
        r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--median-factor", bad],
                           capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--median-factor" in r.stderr, (bad, r.stderr)
    from icp_amd import register
    assert inspect.signature(register.register_clouds).parameters["median_factor"].default is None


def test_example_command_line_accepts_the_option():
    import subprocess
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    for bad in ("0", "-1", "nan", "inf"):
        r = subprocess.run([exe, "--median-factor", bad], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--median-factor: F must be finite and > 0" in r.stderr, (bad, r.stderr)


def test_memory_object_and_layout():
    """Memory.MEDIAN is ICP_MEM_MEDIAN, in front of ICP_MEM_COUNT_."""
    import re
    import icp_amd
    text = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    assert int(re.search(r"ICP_MEM_MEDIAN\s*=\s*(\d+)", text).group(1)) == icp_amd.Memory.MEDIAN == 30
    assert text.index("ICP_MEM_MEDIAN") < text.index("ICP_MEM_COUNT_")
