"""Golden fixture of the workspace sizes: what ``lcfe_workspace_bytes`` and ``lcfe_workspace_bytes_for`` of a build
return over a grid of masks and batch sizes -> ``tests/golden/workspace_bytes.json``.

Recorded from the build BEFORE the workspace layout moved into ``csrc/workspace.hpp`` (the sizes are part of the
contract with callers that allocate the workspace themselves), so run it against that build:

    LCFE_LIB_PATH=/path/to/the/old/liblcfe.so python tests/golden/make_workspace_golden.py

No GPU is needed: the two functions are host arithmetic.  ``tests/test_workspace_cpu.py`` walks the same grid.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

N_OBJ = [0, 1, 7, 1000]
N_POINTS = [0, 1, 63, 120000]
MAX_LEN = [0, 128, 767, 768, 1024, 1025, 2048, 2049, 16384, 20000]
DEFAULT_MASK = 0xFF                    # sets 0..7: the benchmark's workload


def masks(registry):
    """Every set alone, the default eight sets, every set of the registry."""
    bits = [bit for bit, _, _, _ in registry]
    every = 0
    for b in bits:
        every |= 1 << b
    return [1 << b for b in bits] + [DEFAULT_MASK, every]


def table(lib, mask_list):
    """{mask: {"bytes": [n_obj][n_points], "bytes_for": [n_obj][n_points][max_len]}}"""
    out = {}
    for m in mask_list:
        out[str(m)] = {
            "bytes": [[int(lib.lcfe_workspace_bytes(m, no, npt)) for npt in N_POINTS] for no in N_OBJ],
            "bytes_for": [[[int(lib.lcfe_workspace_bytes_for(m, no, npt, ml)) for ml in MAX_LEN] for npt in N_POINTS]
                          for no in N_OBJ]}
    return out


def main():
    from mallorn_astrophysics_amd import _lib
    lib = _lib.load()
    doc = {"n_obj": N_OBJ, "n_points": N_POINTS, "max_len": MAX_LEN, "sizes": table(lib, masks(_lib.registry()))}
    with open(os.path.join(HERE, "workspace_bytes.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(len(doc["sizes"]), "masks,", _lib.LIB_PATH)


if __name__ == "__main__":
    main()
