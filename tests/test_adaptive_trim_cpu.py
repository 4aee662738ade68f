"""Adaptive trimming: the rule itself (tests/adaptive_trim_ref.py, the restatement the GPU tests compare the device with) on hand-made
arrays — n = 0, 1 and 2, all keys in one bin, ties across a bin edge, denormal and zero geo, pairs that are no candidates, q = 2 and
q = 8, min == max == 1, a cost tie, B_j against exact sums — against its brute-force twin, what it chooses on a 75 % / 25 % mixture,
and the parts of the interface that need no device."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adaptive_trim_ref as ref      # noqa: E402
from adaptive_trim_ref import adaptive_trim_rule, brute_force      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pairs_of_geo(geo):
    """Placeholder PF / PM of the right length and the float32 values themselves: rule_on_geo hands the values to the rule as the pairs' geo."""
    geo = np.asarray(geo, np.float32)
    PF = np.zeros((geo.size, 4), np.float32)
    PM = PF.copy()
    return PF, PM, geo


def rule_on_geo(monkeypatch, geo, W0, lo, hi, q):
    """The rule and its twin fed `geo` directly (geo_of replaced: any float32 pattern, denormals included, can then be a pair's geo)."""
    PF, PM, geo = pairs_of_geo(geo)
    monkeypatch.setattr(ref, "geo_of", lambda a, b: geo)
    W0 = np.asarray(W0, np.float32)
    acc, words = adaptive_trim_rule(PF, PM, W0, lo, hi, q)
    twin = brute_force(PF, PM, W0, lo, hi, q)
    if twin is None:
        assert words.tolist() == [0] * 8 and not acc.any()
    else:
        js, K, r_lo, r_hi, nbins, B = twin
        assert words.tolist() == [((js + 1) << 19) - 1, int(np.count_nonzero((W0 != 0) & np.isfinite(geo))), K, K, js, r_lo, r_hi, nbins], (words, twin[:5])
    return acc, words, twin


def bin_of(x):
    return int(np.float32(x).view(np.uint32)) >> 19


def test_no_candidate(monkeypatch):
    acc, words, _ = rule_on_geo(monkeypatch, [], [], 0.05, 0.95, 3)
    assert acc.size == 0 and words.tolist() == [0] * 8
    acc, words, _ = rule_on_geo(monkeypatch, [1, 2, 3], [0, 0, 0], 0.05, 0.95, 3)
    assert not acc.any() and words.tolist() == [0] * 8


def test_one_and_two_candidates(monkeypatch):
    acc, words, _ = rule_on_geo(monkeypatch, [9.0], [1], 0.05, 0.95, 3)
    assert acc.tolist() == [True] and words.tolist() == [((bin_of(9.0) + 1) << 19) - 1, 1, 1, 1, bin_of(9.0), 1, 1, 1]
    # two far apart: 1 / 1^3 against (1 + 100) / 2^3 — the first alone costs less; r_lo = 1, r_hi = 2
    acc, words, _ = rule_on_geo(monkeypatch, [100.0, 1.0], [1, 1], 0.05, 0.95, 3)
    assert acc.tolist() == [False, True] and words[1:].tolist() == [2, 1, 1, bin_of(1.0), 1, 2, 2]
    # two close: (1 + 1.5) / 8 < 1
    acc, words, _ = rule_on_geo(monkeypatch, [1.5, 1.0], [1, 1], 0.05, 0.95, 3)
    assert acc.tolist() == [True, True] and words[1:].tolist() == [2, 2, 2, bin_of(1.5), 1, 2, 2]


def test_all_keys_in_one_bin(monkeypatch):
    geo = np.float32(4.0) + np.arange(50, dtype=np.float32) * np.float32(2.0 ** -10)
    assert len({bin_of(x) for x in geo}) == 1
    acc, words, _ = rule_on_geo(monkeypatch, geo, np.ones(50), 0.25, 0.5, 4)
    assert acc.all() and words.tolist() == [((bin_of(4.0) + 1) << 19) - 1, 50, 50, 50, bin_of(4.0), 13, 25, 1]      # (j_lo == j_hi)


def test_ties_across_a_bin_edge(monkeypatch):
    """Many equal keys at the last key of a bin and many at the first key of the next: a bin is taken whole or not at all."""
    edge = np.uint32(((bin_of(2.0) + 1) << 19) - 1).view(np.float32)
    nxt = np.uint32((bin_of(2.0) + 1) << 19).view(np.float32)
    geo = np.array([edge] * 6 + [nxt] * 6 + [1e6] * 4, np.float32)
    acc, words, _ = rule_on_geo(monkeypatch, geo, np.ones(16), 0.05, 0.95, 3)
    assert words[2] in (6, 12) and np.count_nonzero(acc) == words[2]
    assert words[2] == 12 and words[4] == bin_of(2.0) + 1 and acc.tolist() == [True] * 12 + [False] * 4


def test_denormal_and_zero_geo(monkeypatch):
    den = np.array([1, 5, 0x7FFFF, 0x80000, 0x7FFFFF], np.uint32).view(np.float32)      # bins 0, 0, 0, 1, 15
    geo = np.concatenate([np.zeros(3, np.float32), den, np.array([1.0, 2.0], np.float32)])
    acc, words, twin = rule_on_geo(monkeypatch, geo, np.ones(10), 0.05, 0.95, 2)
    c, B = ref.table(geo)
    assert c[0] == 6 and c[1] == 1 and c[15] == 1 and B[0] == math.fsum(float(x) for x in geo[:6])
    assert words[4] == 0 and words[2] == 6 and acc.tolist() == [True] * 6 + [False] * 4        # (the cost of bin 0 is ~1e-40)
    acc, words, _ = rule_on_geo(monkeypatch, np.zeros(4, np.float32), np.ones(4), 0.5, 1.0, 3)
    assert acc.all() and words.tolist() == [(1 << 19) - 1, 4, 4, 4, 0, 2, 4, 1]                 # (every cost is +0)


def test_non_candidates_are_left_out(monkeypatch):
    geo = np.array([1, 2, 3, 4, np.nan, np.inf, 5, 6], np.float32)
    W0 = np.array([1, 1, 0, 1, 1, 1, 1, 1], np.float32)
    acc, words, _ = rule_on_geo(monkeypatch, geo, W0, 1.0, 1.0, 3)
    assert words[1] == 5 and acc.tolist() == [True, True, False, True, False, False, True, True]
    acc2, words2, _ = rule_on_geo(monkeypatch, geo, np.where(W0 != 0, -0.25, 0), 1.0, 1.0, 3)      # (any weight != 0 counts)
    assert np.array_equal(words, words2)


@pytest.mark.parametrize("q", [2, 8])
def test_the_powers_at_the_ends(monkeypatch, q):
    rng = np.random.default_rng(0xADA7 + q)
    geo = np.concatenate([rng.gamma(2.0, 4.0, 300), rng.uniform(400, 2000, 100)]).astype(np.float32)
    acc, words, twin = rule_on_geo(monkeypatch, geo, np.ones(400), 0.05, 0.95, q)
    assert words[5] == 21 and words[6] == 380 and words[5] <= words[2] <= 400      # (the fractions are floats: 0.05f 400 = 20.0000003)
    r = np.array([7, 1 << 20], np.int64)
    P = ref.power(r, q)
    assert P[0] == float(7 ** q) and P[1] == float(2 ** (20 * q))


def test_min_and_max_of_one_accept_every_candidate(monkeypatch):
    rng = np.random.default_rng(0xADA8)
    geo = rng.gamma(2.0, 4.0, 257).astype(np.float32)
    W0 = (rng.random(257) < 0.8).astype(np.float32)
    acc, words, _ = rule_on_geo(monkeypatch, geo, W0, 1.0, 1.0, 4)
    n = int(np.count_nonzero(W0))
    assert np.array_equal(acc, W0 != 0) and words[1:4].tolist() == [n, n, n] and words[5:].tolist() == [n, n, 1]


def test_a_cost_tie_goes_to_the_lower_bin(monkeypatch):
    """q = 2: one pair of geo 1 costs 1 / 1, and with three of geo 5 more (another bin) (1 + 15) / 16 = 1 too."""
    geo = np.array([1.0, 5.0, 5.0, 5.0], np.float32)
    acc, words, twin = rule_on_geo(monkeypatch, geo, np.ones(4), 0.05, 1.0, 2)
    assert words[7] == 2 and words[4] == bin_of(1.0) and words[2] == 1 and acc.tolist() == [True, False, False, False]
    geo[0] = np.float32(1.0) + np.float32(2.0 ** -20)                     # (a little more than the tie: the upper bin wins)
    acc, words, twin = rule_on_geo(monkeypatch, geo, np.ones(4), 0.05, 1.0, 2)
    assert words[4] == bin_of(5.0) and words[2] == 4


def test_bin_sums_are_exact(monkeypatch):
    rng = np.random.default_rng(0xADA9)
    geo = rng.gamma(1.5, 30.0, 5000).astype(np.float32)
    PF, PM, geo = pairs_of_geo(geo)
    monkeypatch.setattr(ref, "geo_of", lambda a, b: geo)
    c, B = ref.table(geo)
    twin = brute_force(PF, PM, np.ones(5000, np.float32), 0.05, 0.95, 3)
    assert set(twin[5]) == set(np.nonzero(c)[0].tolist())
    for j, exact in twin[5].items():
        assert B[j] == exact, j
    # (and in another order of arrival)
    perm = rng.permutation(5000)
    c2, B2 = ref.table(geo[perm])
    assert np.array_equal(c, c2) and np.array_equal(B.view(np.uint64), B2.view(np.uint64))


def test_the_integral_form_of_a_bin_sum():
    """What the device keeps per bin — the count and the sum of the keys' low 19 bits — gives B_j exactly, denormals included."""
    rng = np.random.default_rng(0xADAA)
    for e in (0, 1, 100, 140):
        for top in (0, 9, 15):
            j = (e << 4) | top
            low = rng.integers(0, 1 << 19, 1000, dtype=np.uint64)
            keys = ((np.uint64(j) << np.uint64(19)) | low).astype(np.uint32)
            base = ((1 << 23) if e else 0) + (top << 19)
            total = 1000 * base + int(low.sum())
            assert math.ldexp(float(total), max(e, 1) - 150) == math.fsum(float(x) for x in keys.view(np.float32)), (e, top)


@pytest.mark.parametrize("n", [2500, 16384, 16900])
@pytest.mark.parametrize("q", [3, 4, 7])
def test_a_mixture_of_inliers_and_outliers(monkeypatch, n, q):
    """75 % inliers (residuals of 3 mm per axis), 25 % outliers (a surface 150 mm away): the rule keeps 70 - 76 % with no fraction given."""
    rng = np.random.default_rng(0xADAB)
    d = rng.normal(0, 3, (n, 3))
    d[rng.random(n) < 0.25, 2] += 150.0
    PF = np.zeros((n, 4), np.float32)
    PM = np.zeros((n, 4), np.float32)
    PM[:, :3] = d
    acc, words = adaptive_trim_rule(PF, PM, np.ones(n, np.float32), 0.05, 0.95, q)
    assert 0.70 <= words[2] / words[1] <= 0.76, (n, q, words)
    assert brute_force(PF, PM, np.ones(n, np.float32), 0.05, 0.95, q)[:5] == tuple(int(x) for x in (words[4], words[2], words[5], words[6], words[7]))


# ---- the interface that needs no device: the header, the enum, the command lines and the keyword

def test_header_and_memory_object():
    import re
    import icp_amd
    text = open(os.path.join(ROOT, "include", "icp_amd.h")).read()
    assert int(re.search(r"ICP_MEM_TRIM_ADAPTIVE\s*=\s*(\d+)", text).group(1)) == icp_amd.Memory.TRIM_ADAPTIVE == 31
    assert text.index("ICP_MEM_TRIM_ADAPTIVE") < text.index("ICP_MEM_COUNT_")
    for decl in ("int icp_set_adaptive_trimming (icp_handle h, float min_fraction, float max_fraction, uint32_t power);",
                 "int icp_get_adaptive_trimming (icp_handle h, float *min_fraction, float *max_fraction, uint32_t *power);",
                 "int icp_batch_set_adaptive_trimming (icp_batch_handle b, float min_fraction, float max_fraction, uint32_t power);"):
        assert decl in text, decl
    L = icp_amd.lib()
    for name in ("icp_set_adaptive_trimming", "icp_get_adaptive_trimming", "icp_batch_set_adaptive_trimming"):
        assert hasattr(L, name), name
    for cls, name in ((icp_amd.ICP, "set_adaptive_trimming"), (icp_amd.ICP, "adaptive_trimming"), (icp_amd.ICPBatch, "set_adaptive_trimming")):
        assert callable(getattr(cls, name)), name


def test_register_command_line_has_the_option():
    import inspect
    import subprocess
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "--adaptive-trim" in r.stdout
    for bad in ("0:0.5", "0.6:0.5", "0.1:1.5", "0.1:0.9:1", "0.1:0.9:9", "0.1", "nan:0.5", "0.1:0.9:x"):
        r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--adaptive-trim", bad],
                           capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--adaptive-trim" in r.stderr, (bad, r.stderr)
    r = subprocess.run([sys.executable, "-m", "icp_amd.register", "a.bin", "b.bin", "--adaptive-trim", "--trim", "0.5"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "exclude each other" in r.stderr, r.stderr
    from icp_amd import register
    assert inspect.signature(register.register_clouds).parameters["adaptive_trim"].default is None
    assert register._adaptive_trim("0.05:0.95") == (0.05, 0.95, 4) and register._adaptive_trim("0.4:1:3") == (0.4, 1.0, 3)


def test_example_command_line_accepts_the_option():
    import subprocess
    exe = os.path.join(ROOT, "examples", "registration")
    assert os.path.exists(exe), "examples/registration is built by build() / make examples"
    for bad in ("0:0.5", "0.6:0.5", "0.1:1.5", "0.1:0.9:1", "0.1:0.9:9", "nan:0.5", "0.1:0.9:x"):
        r = subprocess.run([exe, "--adaptive-trim", bad], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "--adaptive-trim: MIN:MAX[:Q]" in r.stderr, (bad, r.stderr)
    r = subprocess.run([exe, "--adaptive-trim", "--trim", "0.5"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--adaptive-trim and --trim exclude each other" in r.stderr, r.stderr


def test_the_kernel_uses_no_scratch():
    """Both forms of k_adaptive_trim as the compiler reports them (tools/diag/kernel_resources.py; needs hipcc only): no scratch, and an
    LDS table that fits three times in a CU's 160 KiB."""
    sys.path.insert(0, os.path.join(ROOT, "tools", "diag"))
    from kernel_resources import kernel_resources
    res = dict(kernel_resources("icp_amd/csrc/icp_adaptive_trim.hip"))
    assert len(res) == 2 and all(n.startswith("k_adaptive_trim<") for n in res), sorted(res)      # (one workgroup per registration; many)
    for n, r in res.items():
        assert r["scratch"] == 0 and 3 * r["lds"] <= 160 * 1024, (n, r)
