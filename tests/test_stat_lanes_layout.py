"""The index arithmetic of the statistics lanes kernels (csrc/stat_lanes.hpp: LanesLayout<8>, LanesLayout<16> and the
functions that give a band's rows to its lanes and a row its LDS slot) checked on the CPU: a small host program,
compiled against the same header the device build uses, prints what the functions give for each layout, each CAP the
kernels instantiate, each band and every row count from 0 to the band's capacity + 1.  The rows of a band must land, in
order, in the columns of the band's lanes and nowhere else.  Where the release kernel writes a lane's share or a row's
slot out per layout (its register allocation needs that), the -DLCFE_DEBUG build holds those expressions against these
functions on the device (tests/test_gpu_parity.py::test_statistics_lanes_debug_build)."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (16, 32)
STRIDE_PAD = 1          # StatLanesLds<CAP>::STRIDE = CAP + 1
SRC = r'''
#include <cstdio>
#include "stat_lanes.hpp"
using namespace lcfe;
// per (layout, CAP, band, count): "B lpo cap band parts level capacity count fits h", then per lane of the group
// "L lane band part m bridge", then per position "S pos slot" (slot in units of doubles, column stride CAP + 1)
template <class L> void dump(int cap) {
    for (int band = 0; band < kLanesBands; ++band) {
        const int capacity = lanes_capacity<L>(band, cap), parts = L::parts(band);
        for (int count = 0; count <= capacity + 1; ++count) {
            const bool fits = lanes_band_fits<L>(band, count, cap);       // the kernel's own test
            int hb[kLanesBands] = {0, 0, 0, 0, 0, 0};
            hb[band] = lanes_rows_per_part(count, parts);
            std::printf("B %d %d %d %d %d %d %d %d %d\n", L::LPO, cap, band, parts, lanes_level<L>(band), capacity, count, (int)fits, hb[band]);
            if (!fits) continue;
            for (int lane = 0; lane < L::LPO; ++lane) {
                const int b = L::band_of(lane), part = lanes_part_of<L>(lane);
                const int m = (b == band) ? lanes_part_rows(count, hb[band], part) : 0;
                const bool bridge = b == band && lanes_bridge(count, hb[band], part, parts);
                std::printf("L %d %d %d %d %d\n", lane, b, part, m, (int)bridge);
            }
            for (int pos = 0; pos < count; ++pos) std::printf("S %d %d\n", pos, lanes_slot<L>(band, pos, hb, cap + 1));
        }
    }
}
int main() {
    for (int cap : {16, 32}) { dump<LanesLayout<8>>(cap); dump<LanesLayout<16>>(cap); }
    return 0;
}
'''


def _records():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        open(src, "w").write(SRC)
        subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "mallorn-astrophysics_amd", "csrc"), src, "-o", exe],
                       check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    cases = []
    for line in out.split("\n"):
        v = line.split()
        if not v:
            continue
        if v[0] == "B":
            cases.append({"head": tuple(map(int, v[1:])), "lanes": [], "slots": []})
        else:
            cases[-1]["lanes" if v[0] == "L" else "slots"].append(tuple(map(int, v[1:])))
    return cases


def test_lanes_layouts_place_every_row_once():
    cases = _records()
    seen = set()
    for case in cases:
        lpo, cap, band, parts, level, capacity, count, fits, h = case["head"]
        seen.add((lpo, cap, band))
        stride = cap + STRIDE_PAD
        assert capacity == parts * cap and parts == {8: (1, 1, 2, 2, 1, 1), 16: (2, 2, 4, 4, 2, 2)}[lpo][band]
        assert (1 << level) == parts, "a band of P parts is complete after log2(P) merge levels"
        if count > capacity:
            assert count == parts * cap + 1 and not fits and not case["lanes"], "a band beyond its capacity must be refused"
            continue
        assert count <= parts * cap and fits and len(case["lanes"]) == lpo and len(case["slots"]) == count
        own = [(lane, part, m, bridge) for lane, b, part, m, bridge in case["lanes"] if b == band]
        assert [part for _, part, _, _ in own] == list(range(parts)), "a band's lanes are consecutive, parts ascending"
        assert sum(m for _, _, _, m, _ in case["lanes"]) == count and sum(m for _, _, m, _ in own) == count
        assert all(0 <= m <= cap for _, _, _, m, _ in case["lanes"])
        assert h == -(-count // parts) and all(m == min(max(count - part * h, 0), h) for _, part, m, _ in own)
        assert all(m == 0 and not bridge for _, b, _, m, bridge in case["lanes"] if b != band), "only lanes of the band hold its rows"
        # lane-major, ascending: position p is slot (lane, k) with k < m of that lane, one to one
        want = [lane * stride + k for lane, _, m, _ in own for k in range(m)]
        assert [slot for _, slot in case["slots"]] == want and [pos for pos, _ in case["slots"]] == list(range(count))
        # the pair (last row of a part, first row of the next) exists exactly where the next part has a row; the last row
        # of such a part is followed in LDS by the first slot of the next lane's column
        for i, (lane, _, m, bridge) in enumerate(own):
            nxt = own[i + 1][2] if i + 1 < len(own) else 0
            assert bool(bridge) == (nxt > 0)
            if bridge:
                assert m == h and own[i + 1][0] == lane + 1
    assert seen == {(lpo, cap, band) for lpo in (8, 16) for cap in CAPS for band in range(6)}
