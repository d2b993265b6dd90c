// sequence.hpp -- a CSR batch to the padded tensors the sequence classifiers take (DESIGN "Sequence tensors on the device").
//
// The reference's LightcurveDataset (src/models/lightcurve_dataset.py:79-127, 141-170) does, per object and on the host:
// sort by time, cast to float32, shift the time to start at 0, clean NaN / inf, z-score the flux, truncate to max_length
// rows, pad.  Here one wavefront does one object and streams it from global memory: no buffer holds an object, so a light
// curve may have any length.  Three passes over the rows: (1) is the file order already the time order, the smallest
// float32 time, the sum of the cleaned fluxes; (2) their squared deviations; (3) every row to its place.
//
// Row order: stable by (time, file index), NaN times last -- sort_key() of wave.hpp.  When the file order is already
// non-decreasing (the test of stage_object) row r goes to place r.  Otherwise a row's place is its rank: the number of rows
// with a smaller (key, index), counted by the row's lane over all rows of the object -- n * n / 64 steps a lane, for the
// objects a file holds out of order only; the same loop finds the row's predecessor in time for delta_t.
//
// Arithmetic: float32, operation by operation as numpy evaluates the reference's expressions (the build has
// -ffp-contract=off and correctly rounded division); the mean and the population std are accumulated in fp64 over the
// float32 values of ALL rows and rounded to float32 once.
//
// Templates over the wave policy W as everywhere (wave.hpp): WaveOfBlock on the device -- four objects per workgroup --
// and WaveHost (one lane) in the host build of the tests.
#pragma once
#include "wave.hpp"

namespace lcfe {

struct SeqIn {
    const int64_t* offsets;
    const double* t;
    const double* f;
    const double* e;
    const uint8_t* b;
};
// one row of `features`: 16 bytes, written with one store
struct alignas(16) SeqRow {
    float time, flux, err, delta_t;
};
struct SeqOut {
    SeqRow* features;       // [n_obj, L]
    int64_t* bands;         // [n_obj, L]
    float* mask;            // [n_obj, L]
    int64_t* length;        // [n_obj]
    float* mean;            // [n_obj]
    float* std;             // [n_obj]
};

// delta_t is in units of 30 days (lightcurve_dataset.py:166); the z-score is applied above this std and divides by
// std + SEQ_STD_EPS (lightcurve_dataset.py:108-110)
constexpr float SEQ_DT_UNIT = 30.0f, SEQ_STD_EPS = 1e-6f, SEQ_ERR_FLOOR = 0.01f;

LCFE_FN bool seq_finite(float x) { return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) != 0x7f800000u; }
// np.nan_to_num(float32(flux), nan=0, posinf=0, neginf=0)
LCFE_FN float seq_flux(double f) {
    const float x = (float)f;
    return seq_finite(x) ? x : 0.0f;
}
// np.clip(np.nan_to_num(float32(err), nan=1, posinf=1, neginf=1), 0.01, None)
LCFE_FN float seq_err(double e) {
    const float x = (float)e;
    const float c = seq_finite(x) ? x : 1.0f;
    return (c < SEQ_ERR_FLOOR) ? SEQ_ERR_FLOOR : c;
}

// what every row of an object shares
struct SeqObj {
    float tmin, mean, den;
    bool norm;
};

// the row (t, f, e, b) of an object to place `pos`; t_prev: the time of the row before it in time order (pos > 0)
LCFE_FN void seq_put(const SeqOut& O, int64_t at, int64_t pos, const SeqObj& S, double t, double t_prev, double f, double e, uint8_t b) {
    const float time = (float)t - S.tmin;
    float flux = seq_flux(f), err = seq_err(e), dt = 0.0f;
    if (S.norm) {
        flux = (flux - S.mean) / S.den;
        err = err / S.den;
    }
    if (pos > 0) dt = (time - ((float)t_prev - S.tmin)) / SEQ_DT_UNIT;
    O.features[at + pos] = SeqRow{time, flux, err, dt};
    O.bands[at + pos] = (int64_t)b;
    O.mask[at + pos] = 1.0f;
}

// Object i of the batch to row i of the outputs, L = max_length >= 1 places each.  All lanes of the wave must call it.
template <class W>
LCFE_FN void seq_object(const SeqIn& A, const SeqOut& O, int64_t i, int64_t L, bool normalize) {
    const int lane = W::lane();
    const int64_t r0 = A.offsets[i], n = A.offsets[i + 1] - r0, at = i * L;
    const double* t = A.t + r0;
    const double* f = A.f + r0;
    const double* e = A.e + r0;
    const uint8_t* b = A.b + r0;
    const int64_t len = (n == 0) ? 1 : ((n < L) ? n : L);
    SeqObj S{0.0f, 0.0f, 1.0f, false};
    bool sorted = true;
    if (n > 0) {
        // pass 1: order, first epoch, sum
        double tm = __builtin_inf(), s = 0.0;
        bool ok = true, nan_t = false;
        for (int64_t r = lane; r < n; r += W::LANES) {
            const double tr = t[r];
            const float t32 = (float)tr;
            nan_t = nan_t || (t32 != t32);
            tm = ((double)t32 < tm) ? (double)t32 : tm;
            if (r + 1 < n) ok = ok && (tr <= t[r + 1]);
            s += (double)seq_flux(f[r]);
        }
        sorted = W::all(ok);
        S.tmin = W::any(nan_t) ? (float)qnan() : (float)W::min(tm);        // numpy's min: NaN if any
        const double mean64 = W::sum(s) / (double)n;
        // pass 2: population variance about the fp64 mean
        double q = 0.0;
        for (int64_t r = lane; r < n; r += W::LANES) {
            const double d = (double)seq_flux(f[r]) - mean64;
            q += d * d;
        }
        const float std32 = (float)sqrt(W::sum(q) / (double)n);
        if (normalize && std32 > SEQ_STD_EPS) {
            S.norm = true;
            S.mean = (float)mean64;
            S.den = std32 + SEQ_STD_EPS;
        }
    }
    // pass 3: the rows
    if (n == 0) {
        if (lane == 0) {
            O.features[at] = SeqRow{0.0f, 0.0f, 1.0f, 0.0f};
            O.bands[at] = 1;                                                 // "g-band default" (lightcurve_dataset.py:87)
            O.mask[at] = 1.0f;
        }
    } else if (sorted) {
        for (int64_t p = lane; p < len; p += W::LANES)
            seq_put(O, at, p, S, t[p], (p > 0) ? t[p - 1] : 0.0, f[p], e[p], b[p]);
    } else {
        for (int64_t r = lane; r < n; r += W::LANES) {
            const double tr = t[r];
            const uint64_t kr = sort_key(tr);
            int64_t rank = 0;
            uint64_t kp = 0;
            double tp = 0.0;                                                 // the latest row before this one
            for (int64_t j = 0; j < n; ++j) {
                const double tj = t[j];
                const uint64_t kj = sort_key(tj);
                if (kj < kr || (kj == kr && j < r)) {
                    ++rank;
                    if (kj >= kp) { kp = kj; tp = tj; }
                }
            }
            if (rank < L) seq_put(O, at, rank, S, tr, tp, f[r], e[r], b[r]);
        }
    }
    for (int64_t p = len + lane; p < L; p += W::LANES) {
        O.features[at + p] = SeqRow{0.0f, 0.0f, 1.0f, 0.0f};
        O.bands[at + p] = 0;
        O.mask[at + p] = 0.0f;
    }
    if (lane == 0) {
        O.length[i] = len;
        O.mean[i] = S.mean;
        O.std[i] = S.den;
    }
}

}  // namespace lcfe
