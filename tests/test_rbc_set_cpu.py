"""The table of an RBC set (icp_amd/csrc/icp_rbc_set.h: the 15 buffers, their sizes, set <-> icp_params) as a host program against the
sizes written out by hand at six shapes — `make rbc_set_test` builds tests/cpp/rbc_set_test.cpp (AddressSanitizer + UBSan) and runs it.
No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rbc_set_table_matches_the_sizes_written_out():
    r = subprocess.run(["make", "-C", ROOT, "-s", "rbc_set_test"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "rbc_set_test: 91 checks ok" in r.stdout, r.stdout[-2000:]
