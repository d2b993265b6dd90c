"""Records tests/golden/golden_gp1d_points.npz (arrays only).

(a) Given mode through the reference project's own code: for each fixture band a GaussianProcessRegressor with the fixed
    kernel (optimizer=None) is fitted to the prepared band and read with the reference's ``interpolate_at_times``
    (src/features/gaussian_process.py of the reference checkout, imported here at generation time only: pass its root as
    the first argument).  Rows, theta, query times, mean and std are stored.
(b) scikit-learn's float64 deviation from the long-double reference (tests/gp1d_points_reference.py) per band size, for the
    well-conditioned and the edge theta: what the edge class's tolerances are derived from.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gp1d_points_reference as ref  # noqa: E402
from gp1d_eval_reference import prepare  # noqa: E402

GIVEN = [(5, "well"), (31, "well"), (64, "edge"), (112, "well"), (160, "edge")]


def record(path, reference_root, sizes=ref.SIZES):
    sys.path.insert(0, reference_root)
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    from src.features.gaussian_process import interpolate_at_times

    rows, qs, out = [0], [0], {k: [] for k in ("t", "flux", "err", "q_t", "mean", "std", "theta", "n")}
    for n, cls in GIVEN:
        t, f, e = ref.band_rows(n)
        x, y, e2 = prepare(t, f, e)
        c, ell, s2 = np.exp(ref.CLASSES[cls])
        gp = GaussianProcessRegressor(kernel=ConstantKernel(c, "fixed") * RBF(ell, "fixed") + WhiteKernel(s2, "fixed"), alpha=e2,
                                      optimizer=None).fit(x.reshape(-1, 1), y)
        q = ref.queries(n, 33)
        mean, std = interpolate_at_times(gp, t, q, t.min(), t.max() - t.min())
        for k, v in (("t", t), ("flux", f), ("err", e), ("q_t", q), ("mean", mean), ("std", std)):
            out[k].append(np.asarray(v, np.float64))
        out["theta"].append(ref.CLASSES[cls])
        out["n"].append(n)
        rows.append(rows[-1] + n)
        qs.append(qs[-1] + q.size)
    dev_n = [n for n in sizes if n >= 5]
    dev_mean, dev_var = np.zeros((len(dev_n), 2)), np.zeros((len(dev_n), 2))
    for i, n in enumerate(dev_n):
        for k, cls in enumerate(ref.CLASSES):
            dev_mean[i, k], dev_var[i, k] = ref.sklearn_deviation(n, cls)
            print(f"n {n:4d} {cls}: scikit-learn vs long double: mean {dev_mean[i, k]:.3e} var {dev_var[i, k]:.3e}")
    z = {k: np.concatenate(out[k]) for k in ("t", "flux", "err", "q_t", "mean", "std")}
    z.update(theta=np.array(out["theta"]), n=np.array(out["n"]), row_off=np.array(rows), q_off=np.array(qs), dev_n=np.array(dev_n),
             dev_mean=dev_mean, dev_var=dev_var)
    np.savez(path, **z)
    return z


if __name__ == "__main__":
    record(os.path.join(HERE, ref.FIXTURE), sys.argv[1])
