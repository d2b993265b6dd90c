// sequences.cpp -- TEST INFRASTRUCTURE (tests/test_sequences_cpu.py compiles it with g++ into a temporary directory;
// sequences.mk beside it has the same targets): the template of csrc/sequence.hpp on the one-lane WaveHost policy.  With -DSEQUENCES_MAIN it is a stand-alone
// program (the sanitizer build) that runs a small batch and checks the invariants that need no oracle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mallorn-astrophysics_amd/csrc/sequence.hpp"

using namespace lcfe;

// Host pointers throughout; the outputs as lcfe_sequences_device describes them.
extern "C" void sequences_host(int64_t n_obj, int64_t max_length, int normalize, const int64_t* offsets, const double* t, const double* flux,
                               const double* err, const uint8_t* band, float* features, int64_t* bands, float* mask, int64_t* length,
                               float* mean, float* std) {
    const SeqIn A{offsets, t, flux, err, band};
    const SeqOut O{reinterpret_cast<SeqRow*>(features), bands, mask, length, mean, std};
    for (int64_t i = 0; i < n_obj; ++i) seq_object<WaveHost>(A, O, i, max_length, normalize != 0);
}

#ifdef SEQUENCES_MAIN
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "sequences.cpp:%d: %s\n", __LINE__, #c); return 1; } } while (0)
int main() {
    const int sizes[] = {0, 1, 2, 7, 8, 9, 63, 64, 65, 129, 700, 2049};
    const int n_obj = sizeof sizes / sizeof sizes[0];
    std::vector<int64_t> off(n_obj + 1, 0);
    for (int i = 0; i < n_obj; ++i) off[i + 1] = off[i] + sizes[i];
    const int64_t np = off[n_obj];
    std::vector<double> t(np), f(np), e(np);
    std::vector<uint8_t> b(np);
    uint64_t s = 12345;
    auto next = [&s] { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1p-53; };
    for (int i = 0; i < n_obj; ++i)
        for (int64_t r = off[i]; r < off[i + 1]; ++r) {
            // even objects in time order, odd ones not
            t[r] = (i % 2) ? 60000.0 + 500.0 * next() : 60000.0 + 0.25 * (double)(r - off[i]);
            f[r] = 100.0 * next();
            e[r] = next();
            b[r] = (uint8_t)(r % 6);
        }
    f[off[6] + 2] = qnan();
    e[off[7] + 1] = -__builtin_inf();
    for (int64_t L : {1, 8, 500}) {
        std::vector<SeqRow> feat(n_obj * L);
        std::vector<int64_t> bands(n_obj * L), length(n_obj);
        std::vector<float> mask(n_obj * L), mean(n_obj), sd(n_obj);
        sequences_host(n_obj, L, 1, off.data(), t.data(), f.data(), e.data(), b.data(), &feat[0].time, bands.data(), mask.data(), length.data(),
                       mean.data(), sd.data());
        for (int i = 0; i < n_obj; ++i) {
            const int64_t len = sizes[i] == 0 ? 1 : (sizes[i] < L ? sizes[i] : L);
            CHECK(length[i] == len);
            for (int64_t p = 0; p < L; ++p) {
                const SeqRow& row = feat[i * L + p];
                CHECK(mask[i * L + p] == (p < len ? 1.0f : 0.0f));
                CHECK(row.time >= 0.0f && row.delta_t >= 0.0f && row.err > 0.0f && row.flux == row.flux);
                if (p >= len) CHECK(row.time == 0.0f && row.flux == 0.0f && row.err == 1.0f && row.delta_t == 0.0f && bands[i * L + p] == 0);
                if (p > 0 && p < len) CHECK(row.time >= feat[i * L + p - 1].time);
            }
            CHECK(feat[i * L].time == 0.0f && feat[i * L].delta_t == 0.0f);
        }
    }
    printf("sequences host check OK: %lld input rows\n", (long long)np);
    return 0;
}
#endif
