/*
 * lcfe.h -- C-ABI of the MI355X light-curve feature-extraction engine (liblcfe.so).
 *
 * The reference (MALLORN-astrophysics) has no FFI layer: its hot path is the Python call
 *     extract_*_features(lightcurves_df, [metadata_df], object_ids) -> DataFrame
 * (src/features/statistical.py:135, bazin_fitting.py:254, multiband_gp.py:347, tde_physics.py:377,
 *  colors.py:347, lightcurve_shape.py:335, physics_based.py:461, and the inline decline fits of
 *  scripts/train_v55_powerlaw.py:147-202).  Each of those functions groups the long frame by
 * object and loops over the objects in Python.  The entry points below replace the body of that
 * loop for ALL objects at once: the caller packs the frame into CSR arrays (one slice per object,
 * rows in file order) and receives one row of feature columns per object.  A maintainer binds
 * them with ctypes (INTEGRATION.md shows the stub); no torch types cross this boundary.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on an infrastructure error (HIP failure,
 *     bad argument); the message is available from lcfe_last_error().  Numerical failures of a
 *     fit are NOT errors: they produce NaN columns, exactly as the reference's try/except blocks
 *     do (bazin_fitting.py:168-179, multiband_gp.py:192-193, train_v55_powerlaw.py:191-192).
 *   - all arrays are C-contiguous, caller-owned; the library keeps no pointer after return.
 *   - band codes: 0..5 = u,g,r,i,z,y ; 255 = any other Filter value (counted only by the
 *     all-band statistics, as the reference's per-band filters would skip it).
 *   - integer-valued columns (*_n_obs, peak_band) are returned as exact doubles.
 */
#ifndef LCFE_H
#define LCFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* feature-set ids; a mask is an OR of (1 << id).  Output columns of a multi-set call are the
 * concatenation of the sets' columns in increasing id order. */
enum {
    LCFE_SET_STAT = 0,     /* statistical.py:135-226        123 columns */
    LCFE_SET_BAZIN = 1,    /* bazin_fitting.py:254-288       52 columns */
    LCFE_SET_POWERLAW = 2, /* train_v55_powerlaw.py:147-202  27 columns */
    LCFE_SET_TDE = 3,      /* tde_physics.py:355-411         25 columns */
    LCFE_SET_COLOR = 4,    /* colors.py:108-380              83 columns */
    LCFE_SET_SHAPE = 5,    /* lightcurve_shape.py:177-368    65 columns */
    LCFE_SET_PHYSICS = 6,  /* physics_based.py:292-502       32 columns */
    LCFE_SET_GP2D = 7,     /* multiband_gp.py:292-385        27 columns */
    LCFE_SET_GP1D = 8,     /* gaussian_process.py:173-310    21 columns (per-band scikit-learn GP) */
    LCFE_SET_RESEARCH = 9, /* research_features.py:533-600   40 columns (v115: log-log power law, nuclear proxy,
                              colour at peak, Mexican-hat power spectra, luminosity; reads z) */
    LCFE_SET_ECOLOR = 10,  /* enhanced_colors.py:81-189     45 columns (opt-in: colours at 0..150 days after the g peak) */
    LCFE_SET_DECLINE = 11, /* time_to_decline.py:110-175    36 columns (opt-in: time from the peak to 80..10 % per band) */
    LCFE_NUM_SETS = 12
};
#define LCFE_MASK(id) (1 << (id))
#define LCFE_MASK_ALL ((1 << LCFE_NUM_SETS) - 1)

/* Extension sets.  They are selected like the numbered sets, by LCFE_MASK(id) in the mask of any entry point, and their
 * columns and status words follow those of the numbered sets in increasing id order.  But they are NOT counted by
 * LCFE_NUM_SETS, have no slot in lcfe_stats, and are not part of LCFE_MASK_ALL or lcfe_implemented_mask(): adding one
 * changes neither sizeof(lcfe_stats) nor lcfe_version(), so callers compiled against an older header keep working
 * without a recompile.  Which ones a library has: lcfe_implemented_xmask().  Their kernel times: lcfe_last_ext_profile().
 * One call runs numbered and extension sets together on the same side streams; a mask of extension bits only is valid. */
enum {
    LCFE_XSET_ADVANCED = 12, /* advanced_features.py:476-622   50 columns (opt-in: absolute magnitudes, Mexican-hat power
                                spectra of r and g over all pairs of a band, FLEET widths, pre-peak colours, autocorrelation,
                                early / late ratios, higher-order statistics, peak lags; reads z) */
    LCFE_NUM_XSETS = 1
};

/* Registered sets.  Like the extension sets they are selected by LCFE_MASK(id) in any entry point, are in no table above and
 * in neither implemented mask, and their columns and status words follow those of the extension sets in increasing id
 * order.  Unlike them they are counted by no constant of this header: a caller finds them -- with every numbered and
 * extension set -- through lcfe_set_count() / lcfe_set_info(), and reads their kernel times with lcfe_last_set_profile(), so
 * a later set changes no value an existing caller may have compiled in.  Bit 13 is not assigned and never will be. */
enum {
    LCFE_RSET_CESIUM = 14,  /* cesium_features.py:311-414    80 columns (opt-in: per band Stetson J / K, beyond 1 / 2 sigma, flux
                               percentile ratios, percent amplitude, maximum slope, weighted linear trend, Anderson-Darling;
                               then the J consistency of g, r, i and the mean beyond-1-sigma share; no status words, no z) */
    LCFE_RSET_FOURIER = 15  /* fourier_features.py:16-129    24 columns (opt-in: per band the dominant frequency, its power, the
                               ratio to the mean power and the spectral entropy of the Hann-windowed band interpolated onto at
                               most 128 equidistant times; the band's rows are taken in time order; no status words, no z) */
};

/* Per-call profile, filled when a non-NULL pointer is passed.  kernel_ms[s] is the HIP-event time
 * of feature set s's kernel(s) on the stream they were launched on.  The statistics set (with the
 * shared binning prologue) runs alone; the other sets run concurrently on internal side streams
 * forked from / joined into the caller's stream, so their times overlap (environment variable
 * LCFE_SERIAL=1 serialises them for profiling). */
typedef struct lcfe_stats {
    double kernel_ms[LCFE_NUM_SETS];
    double h2d_ms;          /* host-buffer entry point only */
    double d2h_ms;
    int64_t bytes_in;       /* algorithmic input bytes: 25 * n_points + 8 * (n_obj + 1) [+ 8 * n_obj when a z array is
                               passed: read by LCFE_SET_PHYSICS, LCFE_SET_RESEARCH and LCFE_XSET_ADVANCED] */
    int64_t bytes_out;      /* 8 * n_obj * ncols */
    int32_t launches[LCFE_NUM_SETS];
    int32_t reserved;
} lcfe_stats;

/* 2 since LCFE_NUM_SETS = 12 (lcfe_stats grew): C callers must recompile against this header */
int lcfe_version(void);
/* number of visible HIP devices (0 if none) */
int lcfe_device_count(void);
/* message of the last failing call on this thread ("" if none) */
const char* lcfe_last_error(void);

/* number / name of the output columns of a mask (same order as the reference's DataFrame, see
 * mallorn-astrophysics_amd/columns.py); lcfe_colname returns NULL when j is out of range */
int64_t lcfe_ncols(int mask);
const char* lcfe_colname(int mask, int64_t j);
/* int32 status words per object for a mask: Bazin 6 x (status, nfev), power-law 27 x (status, nfev),
 * GP 4 (status, n_iter, n_eval, n_points), per-band GP 4 (L-BFGS-B evaluations of g, r, i, z; -100: band
 * longer than 159 valid points), research 1 and LCFE_XSET_ADVANCED 1 (0, or -100: the r band spans more days than the
 * set's 1-day grid takes -- 65536 / 4194304 -- and the columns computed on that grid are NaN); 0 for the other sets */
int64_t lcfe_nstatus(int mask);

/*
 * Host-buffer entry point: what extract_*_features binds.  Copies the CSR batch to `device`
 * (-1 = current device), runs the kernels of every set in `mask`, copies results back.
 *   offsets  int64[n_obj+1], offsets[0] == 0, non-decreasing
 *   t, flux, err  float64[offsets[n_obj]]   band  uint8[offsets[n_obj]]
 *   z        float64[n_obj] redshift (used by LCFE_SET_PHYSICS, LCFE_SET_RESEARCH and LCFE_XSET_ADVANCED; NULL or NaN
 *            entries = 0, physics_based.py:348; the advanced set's absolute magnitudes are NaN unless z > 0)
 *   out      float64[n_obj * lcfe_ncols(mask)] row-major
 *   status   int32[n_obj * lcfe_nstatus(mask)] or NULL
 */
int lcfe_extract(int mask, int device, int64_t n_obj, const int64_t* offsets, const double* t,
                 const double* flux, const double* err, const uint8_t* band, const double* z,
                 double* out, int32_t* status, lcfe_stats* prof);

/*
 * Device-resident entry point (bench / multi-GPU path): every pointer is a DEVICE pointer on
 * `device`, kernels are enqueued on `stream` (a hipStream_t; NULL = default stream) and the call
 * returns without synchronising unless `prof` is non-NULL (event times need the stream drained).
 *   max_len    an upper bound of the number of points of any object (selects the LDS tier;
 *              objects longer than the largest tier get NaN rows and status -100)
 *   workspace  device scratch of at least lcfe_workspace_bytes(mask, n_obj, n_points) bytes (ticket
 *              counters, per-tier index lists, GP scratch); owned by the call until its work on
 *              `stream` has completed -- concurrent calls need separate workspaces
 */
size_t lcfe_workspace_bytes(int mask, int64_t n_obj, int64_t n_points);
/* ... plus the slabs of the long-object tier for a batch whose longest light curve has max_len rows: light curves beyond
 * the LDS tiers (2048 rows; 1024 for the object-level fits and the research set; 767 for the 2-D and the per-band GP)
 * run with their working set in global scratch, up to lcfe_max_points() rows / lcfe_gp2d_max_points() valid points
 * (2-D GP) / lcfe_gp1d_max_points() valid points per band (per-band GP).  The per-band GP's slabs are counted only for
 * max_len > 767, so batches of shorter light curves keep the size of lcfe_workspace_bytes().  A call whose workspace
 * holds only lcfe_workspace_bytes() leaves such objects NaN with status -100. */
size_t lcfe_workspace_bytes_for(int mask, int64_t n_obj, int64_t n_points, int64_t max_len);
int lcfe_extract_device(int mask, int device, void* stream, int64_t n_obj, int64_t n_points,
                        int64_t max_len, const int64_t* d_offsets, const double* d_t,
                        const double* d_flux, const double* d_err, const uint8_t* d_band,
                        const double* d_z, double* d_out, int32_t* d_status, void* d_workspace,
                        size_t workspace_bytes, lcfe_stats* prof);

/* lcfe_extract keeps its device staging buffers (one set per device, grown on demand) for later calls;
 * this releases them */
void lcfe_release_buffers(void);

/* largest number of points per object any kernel tier accepts (the long-object tier) */
int64_t lcfe_max_points(void);
/* largest number of VALID points (known band, finite flux and error, error > 0) per object the 2-D GP accepts */
int64_t lcfe_gp2d_max_points(void);
/* largest number of VALID points in one band (g, r, i or z) the per-band GP fits; a band with more gets NaN in its four
 * columns and status -100 in its status word, the other bands of the object are still fitted */
int64_t lcfe_gp1d_max_points(void);
/* mask of the numbered feature sets (ids below LCFE_NUM_SETS) this build of the library implements */
int lcfe_implemented_mask(void);
/* mask of the extension sets (LCFE_XSET_*) this build implements; the two masks share no bit */
int lcfe_implemented_xmask(void);
/* kernel time (HIP events, ms) and launch count of the extension sets of the last lcfe_extract / lcfe_extract_device call
 * this THREAD made with prof != NULL: entry k belongs to extension set LCFE_NUM_SETS + k; sets that were not in that
 * call's mask read 0.  Fills min(n, LCFE_NUM_XSETS) entries of each non-NULL array and returns LCFE_NUM_XSETS. */
int lcfe_last_ext_profile(double* kernel_ms, int32_t* launches, int n);


/* The set registry: every set this build has -- numbered, extension and registered -- in increasing mask-bit order.
 * lcfe_set_info describes entry k (0 <= k < lcfe_set_count()): its mask bit, its name (a static string), the number of its
 * columns and of its status words, each through a pointer that may be NULL; it returns 0, or 1 when k is out of range. */
int lcfe_set_count(void);
int lcfe_set_info(int k, int* bit, const char** name, int* ncols, int* nstatus);
/* kernel time (HIP events, ms) and launch count of the set with mask bit `bit` in the last lcfe_extract / lcfe_extract_device
 * call this THREAD made with prof != NULL (0 for a set that was not in that call's mask); for a numbered set the values of
 * lcfe_stats, for an extension set those of lcfe_last_ext_profile.  Returns 0, or 1 for a bit that is no set. */
int lcfe_last_set_profile(int bit, double* kernel_ms, int32_t* launches);

/*
 * Augmentation on the device (augmentation.py:138-186, LightcurveAugmenter.augment_single): k perturbed copies of every
 * light curve of a device-resident CSR batch, as a CSR batch of n_obj * k objects -- copy c of object i at index i * k + c --
 * that lcfe_extract_device accepts as it is.  Like lcfe_extract_device: every pointer is a DEVICE pointer on `device`, the
 * kernels are enqueued on `stream`, the call does not synchronise and allocates nothing.
 *   plan         seven arrays of n_obj * k entries, entry i * k + c describes copy c of object i; the steps, in this order:
 *     scale        flux *= scale, err *= scale
 *     stretch      t = t_min + (t - t_min) * stretch, t_min the object's smallest time that is not NaN; 1 leaves t as it is
 *     noise_scale  flux += err * noise_scale * N(0, 1); 0 = no noise
 *     dropout      a fraction in [0, 1): max(5, (int64)(n * (1 - dropout))) of the object's n rows are kept, in file order;
 *                  objects of up to 5 rows, and dropout 0, keep every row
 *     shift        t += shift; 0 leaves t as it is
 *     band_noise   non-zero: flux += err * {u 1.5, g 1.0, r 0.8, i 0.9, z 1.1, y 1.3} * 0.3 * N(0, 1); none for band 255
 *     seed         key of the copy's Philox4x32-10 draws; counter (row index in the input object, stream, 0, 0) with
 *                  stream 0 = noise, 1 = dropout keys, 2 = band noise; normals by Box-Muller on words 0 and 1,
 *                  u = (w + 0.5) / 2^32; the rows with the smallest (word 0 << 32 | word 1, row index) are kept
 *   add_flux     optional (NULL: none): added to the flux after the noise step; one entry per CANDIDATE row -- input row r
 *                of copy c of object i at index k * offsets[i] + c * n_i + r
 *   keep         optional (NULL: the Philox selection): non-zero = the candidate row is kept; replaces the dropout step
 *   outputs      offsets_out int64[n_obj * k + 1]; t_out, flux_out, err_out float64 and band_out uint8 of at least
 *                lcfe_augment_capacity(n_points, k) = n_points * k entries (-1: bad arguments); n_points_out int64[1], the
 *                rows written -- or -1 when a dropout entry lies outside [0, 1): then no row is written and offsets_out is void
 *   workspace    device scratch of at least lcfe_augment_workspace_bytes(n_obj, k) bytes (first epochs, partial sums of the
 *                prefix sum), owned by the call until its work on `stream` has completed
 * A light curve may have any number of rows below 2^31 (no buffer holds an object).  Errors (lcfe_last_error): k < 1, negative
 * sizes, a NULL required array, a workspace that is too small.
 */
int64_t lcfe_augment_capacity(int64_t n_points, int k);
size_t lcfe_augment_workspace_bytes(int64_t n_obj, int k);
int lcfe_augment_device(int device, void* stream, int64_t n_obj, int64_t n_points, int k, const int64_t* d_offsets,
                        const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band,
                        const double* d_scale, const double* d_stretch, const double* d_shift, const double* d_noise_scale,
                        const double* d_dropout, const uint8_t* d_band_noise, const uint64_t* d_seed,
                        const double* d_add_flux, const uint8_t* d_keep, int64_t* d_offsets_out, double* d_t_out,
                        double* d_flux_out, double* d_err_out, uint8_t* d_band_out, int64_t* d_n_points_out,
                        void* d_workspace, size_t workspace_bytes);

/*
 * The augmentation recipes of gp_augmentation.py (Boone: time shift, sparsening, S/N degradation) and of
 * plasticc_augmentation.py (redshift dilation and dimming, per-band skew, quality degradation): lcfe_augment_device with five
 * more arguments.  Per kept row, in this order (multiplies and adds are never fused):
 *   1. flux *= scale, err *= scale                       2. the stretch             3. flux += err * noise_scale * N(0, 1)
 *      (stream 0), then flux += add_flux
 *   4. band b < 6: flux *= band_scale[b], err *= band_scale[b]; a row of filter 255 is left as it is
 *   5. the dropout selection (stream 1), keeping per keep_rule
 *        0  max(5, (int64)(n * (1 - dropout))) rows, objects of up to 5 rows whole -- the rule of lcfe_augment_device
 *        1  n - (int64)(n * dropout) rows, no floor (gp_augmentation.py:60-61)
 *   6. err *= err_boost                                  7. flux += err * noise2_scale * N(0, 1) with the boosted err, drawn
 *      from stream 3 -- counter (row index in the input object, 3, 0, 0), the same Box-Muller --, then flux += add_flux2
 *   8. the shift                                         9. the band noise
 *   band_scale    float64[n_obj * k, 6] (u g r i z y), err_boost and noise2_scale float64[n_obj * k]; NULL = neutral (1, 1, 0)
 *   add_flux2     optional, per candidate row like add_flux
 * With the three arrays and add_flux2 NULL (or neutral) and keep_rule 0 the output is that of lcfe_augment_device, byte for
 * byte.  Capacity, workspace and outputs as there; errors as there, plus a keep_rule other than 0 and 1.
 */
int lcfe_augment_recipe_device(int device, void* stream, int64_t n_obj, int64_t n_points, int k, const int64_t* d_offsets,
                               const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band,
                               const double* d_scale, const double* d_stretch, const double* d_shift, const double* d_noise_scale,
                               const double* d_dropout, const uint8_t* d_band_noise, const uint64_t* d_seed,
                               const double* d_band_scale, const double* d_err_boost, const double* d_noise2_scale, int keep_rule,
                               const double* d_add_flux, const uint8_t* d_keep, const double* d_add_flux2, int64_t* d_offsets_out,
                               double* d_t_out, double* d_flux_out, double* d_err_out, uint8_t* d_band_out, int64_t* d_n_points_out,
                               void* d_workspace, size_t workspace_bytes);

/*
 * Sequence tensors on the device (models/lightcurve_dataset.py:79-127, 141-170, LightcurveDataset): a device-resident CSR
 * batch -- a staged one or the output of lcfe_augment_device -- to the padded float32 inputs of the sequence classifiers.
 * No feature set: no mask bit, no columns.  Like lcfe_extract_device: every pointer is a DEVICE pointer on `device`, the
 * kernel is enqueued on `stream`, the call does not synchronise and allocates nothing.
 * Per object of n rows, with L = max_length:
 *   order     by (time, file index) over all bands, NaN times last; the first min(n, L) rows are kept
 *   time      float32(t) - min over all n rows of float32(t), in float32
 *   flux      float32(flux), NaN / +-inf -> 0; err: float32(err), NaN / +-inf -> 1, then max(err, 0.01f)
 *   z-score   mean and population std of the cleaned float32 flux over ALL n rows, accumulated in fp64 and rounded to
 *             float32 once; if `normalize` is non-zero and std > 1e-6f: flux = (flux - mean) / (std + 1e-6f),
 *             err = err / (std + 1e-6f), in float32
 *   delta_t   0 for the first row, (time[i] - time[i - 1]) / 30.0f after it
 *   padding   time 0, flux 0, err 1, delta_t 0, band 0, mask 0
 *   n == 0    length 1, row 0 = (0, 0, 1, 0), band 1, mask 1
 * Outputs: features float32[n_obj, L, 4] = (time, flux, err, delta_t), aligned to 16 bytes; bands int64[n_obj, L], the band
 * code of the batch (0..5 = u, g, r, i, z, y; 255 for an unknown filter); mask float32[n_obj, L]; length int64[n_obj];
 * mean, std float32[n_obj]: what the z-score subtracted and divided by (std + 1e-6f), or 0 and 1 where none was applied.
 * A light curve may have any number of rows (no buffer holds an object); one whose file order is not its time order costs
 * n * n / 64 steps.  workspace: at least lcfe_sequences_workspace_bytes(n_obj, n_points, max_len) bytes, max_len the rows
 * of the longest object; this version needs none (0 bytes: `workspace` may be NULL).  Errors (lcfe_last_error):
 * max_length < 1, negative sizes, a NULL or misaligned required array, a workspace that is too small.
 */
size_t lcfe_sequences_workspace_bytes(int64_t n_obj, int64_t n_points, int64_t max_len);
int lcfe_sequences_device(int device, void* stream, int64_t n_obj, int64_t n_points, int64_t max_length, int normalize,
                          const int64_t* d_offsets, const double* d_t, const double* d_flux, const double* d_err,
                          const uint8_t* d_band, float* d_features, int64_t* d_bands, float* d_mask, int64_t* d_length,
                          float* d_mean, float* d_std, void* d_workspace, size_t workspace_bytes);

/*
 * The 2-D GP's posterior mean and variance on a caller's grid (multiband_gp.py:196-247: interpolate_multiband with any epoch
 * list, and the variance george's predict returns there): per light curve a regular time x band tensor with its uncertainty.
 * No feature set: no mask bit, no columns.  Like lcfe_extract_device: the batch -- a staged one or the output of
 * lcfe_augment_device -- and every d_ pointer are DEVICE pointers on `device`, the kernels are enqueued on `stream`, the call
 * does not synchronise and allocates nothing.  `bands` is a HOST array.
 *   grid        point (b, k) of a light curve lies at time origin + d_grid_offsets[k] (days, float64[n_times]) and at the
 *               wavelength of band bands[b] (0..5 = u g r i z y); 1 <= n_times <= lcfe_gp2d_grid_max_times() (1024),
 *               1 <= n_bands <= 6, bands distinct
 *   origin      LCFE_GRID_FROM_PEAK   the gp2d set's own peak time, so offsets {0, 20, 50, 100} are the set's epochs
 *               LCFE_GRID_FROM_FIRST  the light curve's first valid observation
 *   d_theta_in  float64[n_obj, 4] = [mean, log c, log M0, log M1] in the set's normalised units (flux over the median |flux|):
 *               "given" mode, one evaluation per light curve and no optimiser; NULL: "fit" mode, the fit of the gp2d set
 *   d_mean      float64[n_obj, n_bands, n_times]: (mean + k*' K^-1 r) * flux_scale
 *   d_var       float64[n_obj, n_bands, n_times] or NULL (the variance passes are then skipped):
 *               (c - k*' (K + diag e2)^-1 k*) * flux_scale^2 -- no white noise on k(x*, x*), no clamp at 0, as george
 *   d_theta_out float64[n_obj, 4]: the parameters the grid was evaluated at
 *   d_row27     float64[n_obj, 27] or NULL, fit mode only: the gp2d set's row, byte for byte
 *   d_status    int32[n_obj, lcfe_nstatus(1 << LCFE_SET_GP2D)], the set's words: stop reason (given mode: 0, or 5 for a
 *               non-finite theta_in), iterations, evaluations (given mode: 0), valid points; -100 in word 0: too many rows
 * NaN mean and var: fewer than 10 valid points, a non-finite start or parameter vector, a failed factorisation, no peak row
 * (whatever the origin), more valid points than lcfe_gp2d_max_points().
 * workspace: lcfe_gp2d_grid_workspace_bytes(n_obj, n_points, max_len) bytes, max_len the rows of the longest light curve.
 * Errors (lcfe_last_error; nothing is enqueued): sizes or bands outside the limits above, an unknown origin, a NULL
 * required array, d_row27 in given mode, a workspace that is too small.
 */
#define LCFE_GRID_FROM_PEAK 0
#define LCFE_GRID_FROM_FIRST 1
int64_t lcfe_gp2d_grid_max_times(void);
size_t lcfe_gp2d_grid_workspace_bytes(int64_t n_obj, int64_t n_points, int64_t max_len);
int lcfe_gp2d_grid_device(int device, void* stream, int64_t n_obj, int64_t n_points, int64_t max_len, const int64_t* d_offsets,
                          const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band, int n_times,
                          const double* d_grid_offsets, int origin, int n_bands, const int* bands, const double* d_theta_in,
                          double* d_mean, double* d_var, double* d_theta_out, double* d_row27, int32_t* d_status,
                          void* d_workspace, size_t workspace_bytes);

/*
 * The same posterior at scattered points: per light curve a list of (t*, lambda*) pairs, lambda* ANY positive wavelength in
 * Angstrom (a band's wavelength reproduces the grid; 5500 lies between g and r).  Everything lcfe_gp2d_grid_device says about
 * the batch, the stream, theta_in / theta_out, row27, status, the NaN rules and the denormalisation holds here; the stage is
 * the grid's with another column source ("Posterior at points").
 *   d_q_off     int64[n_obj + 1], DEVICE: light curve i owns the points d_q_off[i] .. d_q_off[i + 1]; ascending from 0 to nq.
 *               A light curve may own no point: it is fitted (row27, theta_out, status) and writes nothing else.
 *               The call copies this array to the host ONCE, synchronising `stream`, before anything is enqueued: a list that
 *               does not start at 0, descends or does not end at nq is an error, not an out-of-bounds store.  It is the only
 *               synchronisation of the call.
 *   d_q_t       float64[nq]: days from the origin (LCFE_GRID_FROM_PEAK / LCFE_GRID_FROM_FIRST, the grid's two origins)
 *   d_q_lam     float64[nq]: Angstrom
 *   want_var    0: the variance passes are skipped and d_var is not touched
 *   d_mean, d_var   float64[nq]
 * A point with a non-finite time, or a wavelength that is non-finite or <= 0, is NaN in mean and var and leaves every other
 * point what it is without it.  A light curve without a GP (see above) is NaN at all its points.
 * workspace: lcfe_gp2d_points_workspace_bytes_for(n_obj, n_points, max_len) bytes.
 * Errors (lcfe_last_error; nothing is enqueued): an unknown origin, a negative size, a NULL required array, d_row27 in given
 * mode, a workspace that is too small, a d_q_off as described.
 */
size_t lcfe_gp2d_points_workspace_bytes_for(int64_t n_obj, int64_t n_points, int64_t max_len);
int lcfe_gp2d_points_device(int device, void* stream, int64_t n_obj, int64_t n_points, int64_t max_len, const int64_t* d_offsets,
                            const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band, int64_t nq,
                            const int64_t* d_q_off, const double* d_q_t, const double* d_q_lam, int origin, const double* d_theta_in,
                            int want_var, double* d_mean, double* d_var, double* d_theta_out, double* d_row27, int32_t* d_status,
                            void* d_workspace, size_t workspace_bytes);

/*
 * Posterior mean and standard deviation of the PER-BAND GP of set `gp1d` at a caller's times ("Per-band
 * GP posterior"; reference: gaussian_process.py, interpolate_at_times -> predict(return_std=True)).  No set, no mask bit:
 * an entry point of its own beside lcfe_gp2d_points_device.  Batch arguments as lcfe_extract_device.
 *   d_q_off     int64[n_obj + 1], DEVICE: light curve i owns the queries d_q_off[i] .. d_q_off[i + 1], in any order; checked
 *               on the host as lcfe_gp2d_points_device checks its list (ONE synchronisation of `stream`)
 *   d_q_t       float64[nq]: MJD, the light curve's own time axis
 *   d_q_band    uint8[nq]: 1..4 = g, r, i, z
 *   d_theta_in  float64[n_obj][4][3] (log c, log l, log s2) per band: given mode -- no optimiser, one evaluation; a non-finite
 *               theta skips the band.  NULL: fit mode -- the set's own fit, then one evaluation at the winning theta
 *   d_mean, d_std   float64[nq], in the caller's query order, in the reference's units (standardised flux):
 *               x* = clip((t* - t_min) / t_range, 0, 1), mean = k*' K^-1 y, std = sqrt(max(c + s2 - k*' K^-1 k*, 0))
 *   d_theta_out float64[n_obj][4][3]: the theta the posterior was read at (fit mode: the best of the four runs)
 *   d_norm      float64[n_obj][4][4]: (t_min, t_range, f_mean, f_std) per band; flux = mean f_std + f_mean
 *   d_cols      float64[n_obj][16]: the four per-band columns of set `gp1d` (fit mode: the set's own bytes)
 *   d_status    int32[n_obj][4]: the set's status words (given mode: 1 evaluation)
 * NaN, never an error: a band the reference does not fit, a band of more than lcfe_gp1d_max_points() valid rows, a query
 * with a non-finite time or a band code outside 1..4 -- which leaves every other query what it is without it.
 * workspace: lcfe_gp1d_points_workspace_bytes_for(n_obj, n_points, max_len, nq) bytes.
 * Errors (lcfe_last_error; nothing is enqueued): a negative size, a NULL required array, a workspace that is too small, a
 * d_q_off as described.
 */
size_t lcfe_gp1d_points_workspace_bytes_for(int64_t n_obj, int64_t n_points, int64_t max_len, int64_t nq);
int lcfe_gp1d_points_device(int device, void* stream, int64_t n_obj, int64_t n_points, int64_t max_len, const int64_t* d_offsets,
                            const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band, int64_t nq,
                            const int64_t* d_q_off, const double* d_q_t, const uint8_t* d_q_band, const double* d_theta_in,
                            double* d_mean, double* d_std, double* d_theta_out, double* d_norm, double* d_cols, int32_t* d_status,
                            void* d_workspace, size_t workspace_bytes);

/*
 * GP-resampled copies: the two passes around lcfe_gp2d_points_device (fit mode on the SOURCE batch) that
 * turn the copies an augmentation call produced into copies whose fluxes are drawn from the source's GP posterior at another
 * redshift.  The copies of source o are objects o k .. o k + k - 1 of the copy batch (what lcfe_augment_device writes); a
 * copy keeps its rows (t, band, err).  Device pointers, `stream`, no synchronisation, no workspace.  This recipe has no
 * counterpart in the reference.
 * query: per row r of the copy batch (copy c of source o), s = (1 + z_new[c]) / (1 + z_old[o]):
 *   d_q_t[r] = (t_r - shift[c] - t_ref[o]) / s, d_q_lam[r] = lambda_band(r) / s (3670 4825 6222 7545 8691 9710 A); NaN both for
 *   a row of filter 255.  t_ref: the gp2d set's peak row's time (LCFE_GRID_FROM_PEAK) or the first valid observation
 *   (LCFE_GRID_FROM_FIRST) of the source; NaN where there is none.  d_q_off[o] = d_copy_offsets[o k], int64[n_src + 1]:
 *   point r is row r.  s = 1 and shift = 0 give the row's own time in the origin's frame and its band's wavelength, exactly.
 * write: with mu, var the points stage's outputs at the queries, sd = sqrt(max(var, 0)):
 *   flux = dim (mu + sd n1) + (err noise) n2;  err_out = sqrt(err^2 (1 + noise^2) + (dim sd)^2);  NaN both where mu or var is NaN.
 *   d_n1, d_n2 float64 per row (explicit mode) or both NULL: Philox4x32-10 streams 4 and 5, key d_seed[c], counter (the row's
 *   index in its copy, stream, 0, 0), the Box-Muller of lcfe_augment_device.  d_status_out[c] = word 0 of the source's status.
 * Errors: k < 1, a negative size, an unknown origin, n_copies not a multiple of k, one of n1 / n2 alone, a NULL required array.
 */
int lcfe_gp_resample_query_device(int device, void* stream, int64_t n_src, int k, int origin, const int64_t* d_offsets, const double* d_t,
                                  const double* d_flux, const double* d_err, const uint8_t* d_band, const double* d_z_old,
                                  const int64_t* d_copy_offsets, const double* d_copy_t, const uint8_t* d_copy_band, const double* d_z_new,
                                  const double* d_shift, int64_t* d_q_off, double* d_q_t, double* d_q_lam);
int lcfe_gp_resample_write_device(int device, void* stream, int64_t n_copies, int k, const int64_t* d_copy_offsets, const double* d_copy_err,
                                  const double* d_mean, const double* d_var, const double* d_dim, const double* d_noise, const uint64_t* d_seed,
                                  const double* d_n1, const double* d_n2, const int32_t* d_src_status, int n_status, double* d_flux_out,
                                  double* d_err_out, int32_t* d_status_out);

#ifdef __cplusplus
}
#endif
#endif /* LCFE_H */
