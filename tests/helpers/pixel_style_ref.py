"""numpy restatement of lib/models/pixel_style.py (csrc/pixel_style.hip): the level rule in fp32 as the kernel evaluates it, the integer summary
in the kernel's layout, the three transfers in float64, and the per-element error bar of the kernel's fp32 arithmetic.

THE BAR (u = 2^-24; every term is a magnitude BEFORE cancellation).  The kernel computes, per element,
    d^   = the plane's table entry | fmaf(A^, l, B^) | three nested fmaf over the 3 x 4 matrix K^      (coefficients rounded ONCE from fp64)
    t^   = fl(alpha * d^)
    out^ = fl(t^ * inv^ + x)                                                                              (one fmaf; inv^ = fl(1 / (255 std_c)))
With Mag = |d| (hist), |A l| + |B| (meanstd), sum_b |K_ab l_b| + |K_a3| (cholesky):
    |d^ - d|         <= k_d u Mag     k_d = 1 (the rounded entry), 2 (rounded coefficients + one fmaf), 4 (rounded coefficients + three fmaf,
                                      every partial sum is at most Mag)
    |t^ inv^ - term| <= alpha inv k_d u Mag + 2 u |term|          (the product's rounding, the rounded constant), term = alpha d inv
    |out^ - out|     <= the above + u (|x| + |term|)               (the final rounding)
so   bar = u (k_d alpha inv Mag + 3 |term| + |x|) (1 + 2^-20) + alpha inv (2^-32 Mag + 2^-40).
The factor 1 + 2^-20 covers the products of two roundings.  The last term is the float64 side: this helper and the kernel evaluate the same
real-valued formulas in float64 in different orders - a handful of operations on values up to 256 for the table (2^-40 levels), and for the
covariance forms an error amplified by the condition of Sigma + eps I, at most (0.75 + eps) / eps < 2^17 at eps = 1e-5 (2^-53 2^17 2^4 = 2^-32 of
Mag).  The clamp is monotone and 1-Lipschitz: it keeps the bar."""
import numpy as np

U = 2.0 ** -24
TIE_MARGIN = 2.0 ** -10
K_D = {"hist": 1, "meanstd": 2, "cholesky": 4}


def norm(C, mean=None, std=None):
    """(mean, std) as float32 [1, C, 1, 1]: the values the kernel reads (0 and 1 without normalisation)."""
    mu = np.zeros(C, np.float32) if mean is None else np.asarray(mean, np.float32)
    sd = np.ones(C, np.float32) if std is None else np.asarray(std, np.float32)
    assert mu.shape == (C,) and sd.shape == (C,)
    return mu.reshape(1, C, 1, 1), sd.reshape(1, C, 1, 1)


def from_bytes(b, mean=None, std=None):
    """uint8 [N, C, H, W] -> float32 through the project's normalisation: (b / 255 - mean) / std in fp32 (ToTensor, then Normalize)."""
    mu, sd = norm(b.shape[1], mean, std)
    return ((b.astype(np.float32) / np.float32(255.0) - mu) / sd).astype(np.float32)


def levels(x, mean=None, std=None):
    """int64 levels of float32 [N, C, H, W]: rint(fmaf(x, std, mean) * 255) in fp32, clamped before the cast.  The fused multiply-add is the
    exact product (48 bits: exact in float64) plus mean, rounded to float64 and then to fp32."""
    assert x.dtype == np.float32
    mu, sd = norm(x.shape[1], mean, std)
    with np.errstate(invalid="ignore", over="ignore"):
        r = (x.astype(np.float64) * sd.astype(np.float64) + mu.astype(np.float64)).astype(np.float32)
        v = np.rint(r * np.float32(255.0))
        v = np.fmin(np.fmax(v, np.float32(0.0)), np.float32(255.0))           # (fmax / fmin drop a NaN, as fmaxf / fminf do)
    return v.astype(np.int64)


def assert_clear_of_ties(x, mean=None, std=None):
    """No finite pixel within 2^-10 of a half level: a fused or unfused evaluation moves the value by an ulp, which must not decide a level."""
    mu, sd = norm(x.shape[1], mean, std)
    v = (x.astype(np.float64) * sd.astype(np.float64) + mu.astype(np.float64)) * 255.0
    v = v[np.isfinite(v) & (np.abs(v) < 1e6)]
    dist = np.abs(v - np.floor(v) - 0.5)
    assert dist.size == 0 or dist.min() > TIE_MARGIN, f"a pixel sits {dist.min():.3e} levels from a half level"


def words(C):
    return C * 256 + (8 if C == 3 else 0)


def histograms(lv):
    """int64 [N, C, 256] of levels [N, C, H, W]"""
    N, C = lv.shape[:2]
    return np.stack([np.stack([np.bincount(lv[n, c].ravel(), minlength=256) for c in range(C)]) for n in range(N)]).astype(np.int64)


def cross_sums(lv):
    """int64 [N, 3]: sum l_0 l_1, sum l_0 l_2, sum l_1 l_2"""
    f = lv.reshape(lv.shape[0], 3, -1)
    return np.stack([(f[:, 0] * f[:, 1]).sum(1), (f[:, 0] * f[:, 2]).sum(1), (f[:, 1] * f[:, 2]).sum(1)], axis=1).astype(np.int64)


def summary(x, mean=None, std=None):
    """int32 [N, words(C)] in the kernel's layout (include/udapose.h)"""
    lv = levels(x, mean, std)
    N, C = lv.shape[:2]
    out = np.zeros((N, words(C)), np.int32)
    out[:, :C * 256] = histograms(lv).reshape(N, C * 256).astype(np.int32)
    if C == 3:
        out[:, 768:774] = np.ascontiguousarray(cross_sums(lv)).view(np.int32).reshape(N, 6)       # (little endian: low word first)
    return out


# ---- "hist" ---------------------------------------------------------------------------------------------------------------------------------

def hist_targets_int(hc, hs):
    """float64 [256]: T(k) for the occupied content levels k (nan elsewhere), the integer statement: cumulative COUNTS decide the segment."""
    Cc, Cs = np.cumsum(hc), np.cumsum(hs)
    occ = np.flatnonzero(hs)
    T = np.full(256, np.nan)
    for k in np.flatnonzero(hc):
        q = int(Cc[k])
        if q < Cs[occ[0]]:
            T[k] = occ[0]
        elif q >= Cs[occ[-1]]:
            T[k] = occ[-1]
        else:
            j = int(np.searchsorted(Cs[occ], q, side="right")) - 1
            a, b = int(Cs[occ[j]]), int(Cs[occ[j + 1]])
            T[k] = occ[j] + (q - a) / (b - a) * (occ[j + 1] - occ[j])
    return T


def hist_targets_interp(hc, hs):
    """The same by scikit-image's match_histograms recipe in float64: unique values and counts, cumsum / size, np.interp."""
    src_values, tmpl_values = np.flatnonzero(hc), np.flatnonzero(hs)
    src_q = np.cumsum(hc[src_values]) / hc.sum()
    tmpl_q = np.cumsum(hs[tmpl_values]) / hs.sum()
    T = np.full(256, np.nan)
    T[src_values] = np.interp(src_q, tmpl_q, tmpl_values.astype(np.float64))
    return T


def match_histograms_plane(c, s):
    """skimage.exposure.match_histograms of one integer-valued plane onto another, from the pixels (np.unique), float64."""
    src_values, src_idx, src_counts = np.unique(c.ravel(), return_inverse=True, return_counts=True)
    tmpl_values, tmpl_counts = np.unique(s.ravel(), return_counts=True)
    src_q = np.cumsum(src_counts) / c.size
    tmpl_q = np.cumsum(tmpl_counts) / s.size
    return np.interp(src_q, tmpl_q, tmpl_values.astype(np.float64))[src_idx].reshape(c.shape)


def cdf_step_violations(out_levels, hc, hs):
    """Histogram matching at alpha = 1, read off the OUTPUT's levels: with Co, Cc, Cs the cumulative counts of output, content and style, p0(v) the
    last occupied style level <= v and n1(v) the first one > v, every level v has
        Co[v] <= Cs[n1(v)]  (the total when there is none),   and the smallest content count Cc[k] > Co[v] is >= Cs[p0(v)]  (0 when there is none):
    the output's cumulative histogram stays within one occupied style level of the style's, up to the content's own granularity (pixels of one
    content level move together).  Returns the number of levels that break either."""
    Co, Cc, Cs = np.cumsum(np.bincount(out_levels.ravel(), minlength=256)), np.cumsum(hc), np.cumsum(hs)
    occ = np.flatnonzero(hs)
    bad = 0
    for v in range(256):
        above, below = occ[occ > v], occ[occ <= v]
        hi = Cs[above[0]] if above.size else Cs[-1]
        lo = Cs[below[-1]] if below.size else 0
        nxt = Cc[Cc > Co[v]]
        bad += int(Co[v] > hi) + int(nxt.size > 0 and nxt.min() < lo)
    return bad


# ---- the transfers in float64 ------------------------------------------------------------------------------------------------------------------

def _moments(lv):
    """raw-unit mean [C] and unbiased covariance [C, C] of one sample's levels [C, H, W]"""
    f = lv.reshape(lv.shape[0], -1).astype(np.float64) / 255.0
    return f.mean(axis=1), np.atleast_2d(np.cov(f, ddof=1))


def shift(lc, ls, mode, eps=1e-5):
    """(d, Mag) float64 [N, C, H, W]: d = T - l per pixel of the content levels lc towards the style levels ls, and the magnitude of the terms
    d is added up from (module docstring)."""
    N, C = lc.shape[:2]
    d, mag = np.zeros(lc.shape), np.zeros(lc.shape)
    if mode == "hist":
        hc, hs = histograms(lc), histograms(ls)
        for n in range(N):
            for c in range(C):
                T = hist_targets_interp(hc[n, c], hs[n, c])
                d[n, c] = T[lc[n, c]] - lc[n, c]
        return d, np.abs(d)
    for n in range(N):
        mu_c, S_c = _moments(lc[n])
        mu_s, S_s = _moments(ls[n])
        l = lc[n].astype(np.float64)
        if mode == "meanstd":
            for c in range(C):
                sc, ss = np.sqrt(S_c[c, c] + eps), np.sqrt(S_s[c, c] + eps)
                d[n, c] = 255.0 * ((l[c] / 255.0 - mu_c[c]) / sc * ss + mu_s[c]) - l[c]          # calc_mean_std / adain, on pixels
                g = ss / sc
                mag[n, c] = np.abs((g - 1.0) * l[c]) + abs(255.0 * (mu_s[c] - g * mu_c[c]))
        else:
            assert mode == "cholesky" and C == 3
            L_c, L_s = np.linalg.cholesky(S_c + eps * np.eye(3)), np.linalg.cholesky(S_s + eps * np.eye(3))
            M = L_s @ np.linalg.inv(L_c)
            T = 255.0 * (np.einsum("ab,bhw->ahw", M, l / 255.0 - mu_c.reshape(3, 1, 1)) + mu_s.reshape(3, 1, 1))
            d[n] = T - l
            K, k3 = M - np.eye(3), 255.0 * (mu_s - M @ mu_c)
            mag[n] = np.einsum("ab,bhw->ahw", np.abs(K), l) + np.abs(k3).reshape(3, 1, 1)
    return d, mag


def transfer(xc, xs, mode, alpha, clamp=None, mean=None, std=None, eps=1e-5):
    """(out, bar) float64: the transfer of float32 content xc towards style xs, and the per-element bar of the module docstring."""
    d, mag = shift(levels(xc, mean, std), levels(xs, mean, std), mode, eps)
    return finish(xc, d, mag, mode, alpha, clamp, std)


def finish(xc, d, mag, mode, alpha, clamp=None, std=None):
    """(out, bar) from shift()'s (d, Mag): out = x + alpha d inv_c, clamped.  alpha is taken as the fp32 value the kernel reads."""
    C = xc.shape[1]
    _, sd = norm(C, None, std)
    inv = 1.0 / (255.0 * sd.astype(np.float64))
    a = float(np.float32(alpha))
    x = xc.astype(np.float64)
    term = a * d * inv
    out = x + term
    bar = U * (K_D[mode] * a * inv * mag + 3.0 * np.abs(term) + np.abs(x)) * (1.0 + 2.0 ** -20) + a * inv * (2.0 ** -32 * mag + 2.0 ** -40)
    if clamp is not None:
        lo = np.asarray(clamp[0], np.float32).astype(np.float64).reshape(1, C, 1, 1)
        hi = np.asarray(clamp[1], np.float32).astype(np.float64).reshape(1, C, 1, 1)
        out = np.maximum(np.minimum(out, hi), lo)
    return out, bar
