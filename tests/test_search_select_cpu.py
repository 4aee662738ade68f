"""The selection of the dense search kernel (icp_amd/csrc/icp_search_select.h: tile, SINGLE / MASKED, S2W, grid) as a host program
against the rule written out as a table — `make search_select_test` builds tests/cpp/search_select_test.cpp and runs it.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_selection_matches_the_rule_as_a_table():
    r = subprocess.run(["make", "-C", ROOT, "-s", "search_select_test"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "search_select_test: 128 cases ok" in r.stdout, r.stdout[-2000:]
