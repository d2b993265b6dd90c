// augment.hpp -- light-curve augmentation on a CSR batch: K perturbed copies of every object (DESIGN "Augmentation").
//
// The six steps of the reference's LightcurveAugmenter.augment_single (src/features/augmentation.py:138-186), in its order:
// flux scale, time stretch about the object's first epoch, noise in units of the scaled error, observation dropout, time
// shift, band noise.  The reference draws every number from one numpy RandomState, row after row and copy after copy; here
// every draw is a pure function of (the copy's 64-bit seed, the row's index in the INPUT object, a stream id) through
// Philox4x32-10, so a row's values depend on neither the lane nor the workgroup nor the batch it is computed in.
//
// The recipe pass (RECIPE = true) is the same routine with the steps the Boone recipe (src/features/gp_augmentation.py) and
// the PLAsTiCC recipe (src/features/plasticc_augmentation.py) add: a per-band factor on flux and error after the noise, an
// error boost and a second noise term (stream 3) after the dropout, and Boone's keep count.  Every new step has a neutral
// value; with all of them neutral the recipe pass writes the bytes of the plain one.
//
// Templates over the wave policy W as everywhere (wave.hpp): AugWave on the device -- one wavefront per input object, four
// objects per workgroup -- and WaveHost (one lane) in the host build of the tests.
#pragma once
#include "wave.hpp"

namespace lcfe {

// ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
LCFE_FN void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

enum { AUG_STREAM_NOISE = 0, AUG_STREAM_DROPOUT = 1, AUG_STREAM_BAND = 2, AUG_STREAM_NOISE2 = 3 };

// the four words of (seed, row, stream): counter = (row, stream, 0, 0), key = the seed's low and high word
LCFE_FN void aug_words(uint64_t seed, uint32_t row, uint32_t stream, uint32_t (&w)[4]) {
    philox4x32_10(row, stream, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
}

// Box-Muller on two words; u = (w + 0.5) / 2^32 lies in (0, 1), so the logarithm never sees 0
LCFE_FN double aug_normal_of(uint32_t w0, uint32_t w1) {
    const double u1 = ((double)w0 + 0.5) * 0x1p-32, u2 = ((double)w1 + 0.5) * 0x1p-32;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
LCFE_FN double aug_normal(uint64_t seed, int64_t row, uint32_t stream) {
    uint32_t w[4];
    aug_words(seed, (uint32_t)row, stream, w);
    return aug_normal_of(w[0], w[1]);
}
// the dropout key of a row: the rows with the smallest (key, row) are kept
LCFE_FN uint64_t aug_key(uint64_t seed, int64_t row) {
    uint32_t w[4];
    aug_words(seed, (uint32_t)row, AUG_STREAM_DROPOUT, w);
    return ((uint64_t)w[0] << 32) | w[1];
}

// rows kept of n by a dropout fraction d in [0, 1): max(5, int(n (1 - d))) (augmentation.py:102); objects of up to 5
// rows -- for fewer than 5 the reference's choice() raises -- and d == 0 keep every row
LCFE_FN int64_t aug_n_keep(int64_t n, double d) {
    if (n <= 5 || d == 0.0) return n;
    const int64_t m = (int64_t)((double)n * (1.0 - d));
    return (m < 5) ? 5 : ((m < n) ? m : n);
}
LCFE_FN bool aug_dropout_valid(double d) { return d >= 0.0 && d < 1.0; }
// the keep rules of a recipe call: 0 the rule above; 1 Boone's n - int(n d) (gp_augmentation.py:60-61), no floor
enum { AUG_KEEP_FLOOR5 = 0, AUG_KEEP_BOONE = 1, AUG_KEEP_RULES = 2 };
LCFE_FN int64_t aug_n_keep_rule(int64_t n, double d, int rule) {
    if (rule == AUG_KEEP_FLOOR5) return aug_n_keep(n, d);
    const int64_t m = n - (int64_t)((double)n * d);
    return (m < 0) ? 0 : ((m < n) ? m : n);
}

// noise factor of a band in band_specific_noise (augmentation.py:128); an unknown filter gets none
LCFE_FN double aug_band_scale(int b) {
    return (b == 0) ? 1.5 : (b == 1) ? 1.0 : (b == 2) ? 0.8 : (b == 3) ? 0.9 : (b == 4) ? 1.1 : 1.3;
}

// the batch, the plan (one entry per output object i * k + c) and the outputs
struct AugIn {
    const int64_t* offsets;
    const double* t;
    const double* f;
    const double* e;
    const uint8_t* b;
    const double* add_flux;     // optional, per candidate row
    const uint8_t* keep;        // optional, per candidate row
    int k;
    const double* add_flux2;    // recipe pass: optional, per candidate row
};
struct AugPlan {
    const double* scale;
    const double* stretch;
    const double* shift;
    const double* noise_scale;
    const double* dropout;
    const uint8_t* band_noise;
    const uint64_t* seed;
    // recipe pass; a null array is neutral throughout
    const double* band_scale;   // [n_obj * k, 6]
    const double* err_boost;
    const double* noise2_scale;
    int keep_rule;
};
struct AugOut {
    int64_t* offsets;
    double* t;
    double* f;
    double* e;
    uint8_t* b;
};

#if defined(__HIPCC__)
// one wavefront of a larger workgroup with an object of its own (WaveOfBlock), plus the prefix count of the compaction
struct AugWave : WaveOfBlock {
    static __device__ __forceinline__ int prefix(unsigned long long mask) { return WaveDev::prefix(mask); }
};
#endif

LCFE_FN void aug_hist_add(int* slot) {
#if defined(__HIPCC__)
    atomicAdd(slot, 1);
#else
    ++*slot;
#endif
}

// min of t[0..n) that skips NaN, as pandas' Series.min(); NaN for no such row.  Uniform over the wave.
template <class W>
LCFE_FN double aug_tmin(const double* t, int64_t n) {
    double m = __builtin_inf();
    bool have = false;
    for (int64_t r = W::lane(); r < n; r += W::LANES) {
        const double v = t[r];
        if (v == v) { have = true; m = (v < m) ? v : m; }
    }
    m = W::min(m);
    return W::any(have) ? m : qnan();
}

// Pass 1 for input object i: its first epoch, and the row count of each of its k copies into counts[i * k + c].
// Returns false when a copy's dropout fraction lies outside [0, 1).
template <class W>
LCFE_FN bool aug_count_object(const AugIn& A, const AugPlan& P, int64_t i, double* tmin, int64_t* counts) {
    const int64_t r0 = A.offsets[i], n = A.offsets[i + 1] - r0;
    const double tm = aug_tmin<W>(A.t + r0, n);
    if (W::lane() == 0) tmin[i] = tm;
    bool ok = true;
    for (int c = 0; c < A.k; ++c) {
        const int64_t o = i * A.k + c;
        int64_t m;
        if (A.keep) {
            const uint8_t* kp = A.keep + (A.k * r0 + c * n);
            int cnt = 0;
            for (int64_t r = W::lane(); r < n; r += W::LANES) cnt += kp[r] != 0;
            m = W::sum(cnt);
        } else {
            const double d = P.dropout[o];
            ok = ok && aug_dropout_valid(d);
            m = aug_dropout_valid(d) ? aug_n_keep_rule(n, d, P.keep_rule) : 0;
        }
        if (W::lane() == 0) counts[o] = m;
    }
    return ok;
}

// Smallest digit whose inclusive count exceeds r among the 64 bins of `hist` (their total exceeds r), and the count of the
// bins below it.  Uniform over the wave.
template <class W>
LCFE_FN int aug_find_digit(const int* hist, int64_t r, int* below) {
#if defined(__HIPCC__)
    if constexpr (W::LANES == 64) {
        const int lane = W::lane();
        const int h = hist[lane];
        int c = h;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(c, d, 64);
            if (lane >= d) c += u;
        }
        const int dg = __builtin_ctzll(W::ballot((int64_t)c > r));
        *below = __shfl(c - h, dg, 64);
        return dg;
    }
#endif
    int c = 0, dg = 0;
    while (dg < 63 && (int64_t)c + hist[dg] <= r) c += hist[dg++];
    *below = c;
    return dg;
}

// The key of rank `rank` (0-based, rank < n) among the dropout keys of rows 0..n) and the number of keys below it: a radix
// select, most significant digit first, 6 bits a pass -- each pass counts the keys that share the digits found so far into
// 64 bins.  Keys are recomputed, never stored, so the length of an object is not limited by any buffer.  `hist`: 64 words
// the wave owns.
template <class W>
LCFE_FN uint64_t aug_select_key(uint64_t seed, int64_t n, int64_t rank, int* hist, int64_t* n_below) {
    uint64_t found = 0;
    int64_t below = 0, r = rank;
    for (int s = 60; s >= 0; s -= 6) {
        for (int d = W::lane(); d < 64; d += W::LANES) hist[d] = 0;
        W::sync();
        const uint64_t high = (s + 6 >= 64) ? 0ull : (~0ull << (s + 6));
        for (int64_t row = W::lane(); row < n; row += W::LANES) {
            const uint64_t key = aug_key(seed, row);
            if ((key & high) == found) aug_hist_add(&hist[(key >> s) & 63]);
        }
        W::sync();
        int b = 0;
        const int dg = aug_find_digit<W>(hist, r, &b);
        found |= (uint64_t)dg << s;
        r -= b;
        below += b;
        W::sync();
    }
    *n_below = below;
    return found;
}

// Pass 2 for input object i: the rows of its k copies, each compacted in file order at its offset of O.offsets.  RECIPE adds
// the steps of the recipe pass, in the reference's order: the band factor after the first noise term, the error boost and
// the second noise term -- in units of the boosted error -- after the selection.
template <class W, bool RECIPE = false>
LCFE_FN void aug_write_object(const AugIn& A, const AugPlan& P, const AugOut& O, int64_t i, const double* tmin, int* hist) {
    const int lane = W::lane();
    const int64_t r0 = A.offsets[i], n = A.offsets[i + 1] - r0;
    const double tm = tmin[i];
    for (int c = 0; c < A.k; ++c) {
        const int64_t o = i * A.k + c, cand0 = A.k * r0 + c * n;
        const int64_t o0 = O.offsets[o], n_out = O.offsets[o + 1] - o0;
        const double sc = P.scale[o], st = P.stretch[o], sh = P.shift[o], ns = P.noise_scale[o];
        const bool bn = P.band_noise[o] != 0;
        const uint64_t seed = P.seed[o];
        double bs[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0}, eb = 1.0, n2 = 0.0;
        if constexpr (RECIPE) {
            if (P.band_scale)
                for (int j = 0; j < 6; ++j) bs[j] = P.band_scale[o * 6 + j];
            if (P.err_boost) eb = P.err_boost[o];
            if (P.noise2_scale) n2 = P.noise2_scale[o];
        }
        // selection: the caller's flags, or the n_out rows with the smallest (key, row), or every row
        const bool select = !A.keep && n_out < n;
        uint64_t thr = 0;
        int64_t quota = 0;                       // rows kept among those whose key equals the threshold, first rows first
        if (select && n_out > 0) {
            int64_t below = 0;
            thr = aug_select_key<W>(seed, n, n_out - 1, hist, &below);
            quota = n_out - below;
        }
        int64_t run = 0, ties = 0;
        for (int64_t base = 0; base < n; base += W::LANES) {
            const int64_t r = base + lane;
            const bool in = r < n;
            bool kp = in, tie = false;
            if (in && A.keep) kp = A.keep[cand0 + r] != 0;
            if (select) {
                const uint64_t key = in ? aug_key(seed, r) : ~0ull;
                kp = in && key < thr;
                tie = in && key == thr;
                const unsigned long long tmask = W::ballot(tie);
                if (tie) kp = ties + W::prefix(tmask) < quota;
                ties += popcll(tmask);
            }
            const unsigned long long kmask = W::ballot(kp);
            const int64_t pos = run + W::prefix(kmask);
            if (kp && pos < n_out) {
                const int64_t g = r0 + r;
                double t = A.t[g], f = A.f[g] * sc;
                double e = A.e[g] * sc;
                const int b = A.b[g];
                if (st != 1.0) t = tm + (t - tm) * st;
                if (ns != 0.0) f = f + (e * ns) * aug_normal(seed, r, AUG_STREAM_NOISE);
                if (A.add_flux) f = f + A.add_flux[cand0 + r];
                if constexpr (RECIPE) {
                    if (b < 6) {
                        const double s = (b == 0) ? bs[0] : (b == 1) ? bs[1] : (b == 2) ? bs[2] : (b == 3) ? bs[3] : (b == 4) ? bs[4] : bs[5];
                        if (s != 1.0) { f = f * s; e = e * s; }
                    }
                    if (eb != 1.0) e = e * eb;
                    if (n2 != 0.0) f = f + (e * n2) * aug_normal(seed, r, AUG_STREAM_NOISE2);
                    if (A.add_flux2) f = f + A.add_flux2[cand0 + r];
                }
                if (sh != 0.0) t = t + sh;
                if (bn && b < 6) f = f + ((e * aug_band_scale(b)) * 0.3) * aug_normal(seed, r, AUG_STREAM_BAND);
                O.t[o0 + pos] = t;
                O.f[o0 + pos] = f;
                O.e[o0 + pos] = e;
                O.b[o0 + pos] = (uint8_t)b;
            }
            run += popcll(kmask);
        }
    }
}

}  // namespace lcfe
