"""Golden fixture of the launch counts: how many kernels every set enqueues for small batches that end in each of its
tiers -> ``tests/golden/launch_counts.json``.

Recorded on an MI355X from the build BEFORE the launchers moved onto one grid launcher (csrc/workspace.hpp,
``launch_grid``): a launch sequence that loses or gains a launch shows here whatever the outputs look like.

    LCFE_LIB_PATH=/path/to/the/old/liblcfe.so python tests/golden/make_launch_counts_golden.py           # writes the file
    python tests/golden/make_launch_counts_golden.py --print                                              # JSON on stdout

Every set runs alone, with LCFE_SERIAL=1 (read once per process, so this is a process of its own: the test starts it
as a child), over batches of 8 hand-made light curves whose longest has ROWS rows (GP_ROWS for the two GP sets: no long
GP tier, which would take seconds); ``lcfe_last_set_profile`` gives the count.
"""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

ROWS = [100, 200, 400, 800, 1500, 2100]
GP_ROWS = [60, 100, 150, 200, 400, 600]


def batch(longest, seed=11):
    """8 light curves of longest/8, 2 longest/8, .. longest rows (at least 5)."""
    from mallorn_astrophysics_amd import synth
    rng = np.random.default_rng(seed)
    objs = []
    for k in range(1, 9):
        rows = max(5, longest * k // 8)
        t = np.sort(59000 + rng.uniform(0, 800, rows))
        f = 30 * np.exp(-0.5 * ((t - 59300) / 40) ** 2) + rng.normal(0, 1, rows)
        objs.append((t, f, np.full(rows, 1.0), rng.choice(6, rows)))
    return synth.from_objects(objs)


def counts():
    """{set: [launches for each entry of ROWS / GP_ROWS]}"""
    os.environ["LCFE_SERIAL"] = "1"
    from mallorn_astrophysics_amd import _lib
    from mallorn_astrophysics_amd.engine import extract_csr
    lib = _lib.load()
    out = {}
    for bit, name, _, _ in _lib.registry():
        out[name] = []
        for longest in (GP_ROWS if name in ("gp2d", "gp1d") else ROWS):
            lc = batch(longest)
            extract_csr(name, lc, z=lc["z"], return_prof=True)
            nl = ctypes.c_int32()
            assert lib.lcfe_last_set_profile(bit, None, ctypes.byref(nl)) == 0
            out[name].append(nl.value)
    return out


if __name__ == "__main__":
    doc = {"rows": ROWS, "gp_rows": GP_ROWS, "launches": counts()}
    if "--print" in sys.argv:
        print(json.dumps(doc))
    else:
        with open(os.path.join(HERE, "launch_counts.json"), "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(doc)
