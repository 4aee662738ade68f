"""The word areas behind the moments (icp_amd/csrc/icp_kernels.h: icp_mom_layout_of, icp_words and the accessors) as a host program
and a selection's words under both rules, against offsets written out by hand at six shapes, two of them with a key array — `make mom_layout_test` builds
tests/cpp/mom_layout_test.cpp (AddressSanitizer + UBSan) and runs it.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mom_layout_matches_the_offsets_written_out():
    r = subprocess.run(["make", "-C", ROOT, "-s", "mom_layout_test"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "mom_layout_test: 384 checks ok" in r.stdout, r.stdout[-2000:]
