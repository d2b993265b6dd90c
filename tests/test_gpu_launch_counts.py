"""Every set enqueues as many kernels as the build before the one grid launcher did: launch counts of each set alone, with
LCFE_SERIAL=1, over batches that end in each of its tiers, against tests/golden/launch_counts.json
(tests/golden/make_launch_counts_golden.py), exactly."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
with open(os.path.join(GOLDEN, "launch_counts.json")) as f:
    REF = json.load(f)


@pytest.fixture(scope="module")
def launch_counts():
    # LCFE_SERIAL is read once per process: a fresh child
    env = dict(os.environ, LCFE_SERIAL="1")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_launch_counts_golden.py"), "--print"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(REF["launches"]))
def test_launch_counts_match_the_recorded_build(name, launch_counts):
    assert (launch_counts["rows"], launch_counts["gp_rows"]) == (REF["rows"], REF["gp_rows"])
    assert sorted(launch_counts["launches"]) == sorted(REF["launches"])
    print(name, launch_counts["launches"][name], REF["launches"][name])
    assert launch_counts["launches"][name] == REF["launches"][name]
