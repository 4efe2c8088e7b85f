"""Float64 references of Fourier-domain style transfer (csrc/fda.hip, lib.models.fda), their bars, and the seeded inputs of its tests.
CPU and numpy only.  Images are [N, C, H, W]; a spectrum is complex [N, C, 2b+1, b+1], row u + b (u = -b .. b), column v = 0 .. b.

Three forms, all float64:
  fft_form      the textbook pipeline: np.fft.fft2, amplitude and phase, fftshift, the centre (2b+1) x (2b+1) block of the amplitude becomes
                (1 - alpha) A_content + alpha A_style, ifftshift, ifft2, real part.
  low_rank      out = content + IDFT2(dF), dF = alpha (A_s - A_c) G_c / |G_c| on the window (G_c == 0: the phase is 1, np.angle(0) == 0), from
                (2b+1) x (b+1) direct DFT coefficients per plane and a synthesis of the same rank - what the kernels compute.
  raw-space DC  low_rank(mean=, std=): the planes hold (raw - mean_c) / std_c; the DC coefficient's amplitude and phase are formed on
                std_c G[0,0] + mean_c H W and its dF is divided by std_c.  raw_reference() is normalise(fft_form(denormalise(.), denormalise(.))).

Bars.  u = 2^-24.  The kernels' sums, in their order (csrc/fda.hip):
  spectrum   one wave per image row and eight v: a lane adds its products x = l, l + 64, .. in sequence (runs of four: six xor steps join the
             lanes per run, a further run of 256 pixels is added behind - never more than ceil(W / 64) + 6 additions); a work-group adds its
             min(32, H) rows in sequence; a second kernel adds the ceil(H / 32) groups in sequence.  Six more roundings for the two phase tables
             (fp64 rounded to fp32), the products and the complex product's two-term sums:
                 L_spec = ceil(W / 64) + 6 + min(32, H) + ceil(H / 32) + 6
             Every term of either component of G[u, v] is at most |x[y, x]| in magnitude:  E(G) = u L_spec sum|x| per component.
  window     dF = k alpha (A_s - A_c) G_c / |G_c| (k = 1; raw-space DC: k = 1 / std_c on G' = std_c G + mean_c H W with
             E(G') = std_c E(G) + 2 u (std_c |G| + |mean_c| H W)).  A_s and A_c inherit E(G_s) and E(G_c); the unit phase moves by at most
             E(G_c) / |G_c| per unit of E - the phase-conditioning term 2 alpha |A_s - A_c| E(G_c) / |G_c| (zero where E(G_c) is zero: an all-zero
             plane); the fp32 hypot, subtraction, division and products add 6 u alpha (A_s + A_c):
                 E(dF) = k alpha (E(G_s) + E(G_c) + 2 |A_s - A_c| E(G_c) / |G_c| + 6 u (A_s + A_c))
  output     S[y, v] adds 2b+1 terms in sequence, the pixel adds b terms, then the scale, the content and the store:
                 L_out = (2b + 1) + b + 6
             bar[y, x] = u L_out (|content| + sum_w w |dF| / (H W)) + sum_w w E(dF) / (H W),  w = 1 at v = 0 and 2 at v >= 1
             (|Re(a b)| <= |a| |b|, so the moduli are the absolute-value sums of the chain).
The phase term is why the tests keep min |G_c| >= 1e-5 sum|x| over the window (condition(), pick_seed()): below that the bar says nothing."""
import functools

import numpy as np

U32 = 2.0 ** -24
ROWS = 32           # image rows per work-group (FDA_ROWS)
LANES = 64
MIN_CONDITION = 1e-5


def chain_spec(H, W):
    return -(-W // LANES) + 6 + min(ROWS, H) + -(-H // ROWS) + 6


def chain_out(b):
    return (2 * b + 1) + b + 6


def window(H, W, beta):
    return int(np.floor(min(H, W) * beta))


def inputs(shape, seed):
    """(content, style): float32 [N, C, H, W] of O(1) values - a smooth illumination field, a few mid-frequency waves and white noise, with
    a different mean and contrast on the two sides (so that the amplitudes differ in every coefficient)."""
    N, C, H, W = shape
    rng = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    out = []
    for mean, contrast in ((0.45, 0.22), (0.60, 0.35)):
        img = np.empty(shape)
        for n in range(N):
            for c in range(C):
                ph = rng.uniform(0, 2 * np.pi, 4)
                fr = rng.randint(1, 4, 4)
                field = np.sin(2 * np.pi * fr[0] * yy + ph[0]) * np.cos(2 * np.pi * fr[1] * xx + ph[1]) + 0.5 * np.sin(2 * np.pi * (fr[2] * yy + fr[3] * xx) + ph[2])
                img[n, c] = mean + rng.uniform(-0.1, 0.1) + contrast * (0.4 * field + rng.standard_normal((H, W)))
        out.append(img.astype(np.float32))
    return out[0], out[1]


def _twiddles(n, freqs, sign):
    """exp(sign 2 pi i f t / n) as [len(freqs), n], the phase reduced exactly in integers"""
    f = np.asarray(freqs, dtype=np.int64)[:, None]
    t = np.arange(n, dtype=np.int64)[None, :]
    return np.exp(sign * 2j * np.pi * ((f * t) % n) / n)


def spectrum(x, b):
    """complex128 [N, C, 2b+1, b+1]"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    eh = _twiddles(H, np.arange(-b, b + 1), -1.0)        # [2b+1, H]
    ew = _twiddles(W, np.arange(0, b + 1), -1.0)         # [b+1, W]
    return np.matmul(np.matmul(eh, x.astype(np.complex128)), ew.T)


def condition(x, b):
    """min over the window and the planes of |G| / sum|x| (the tests' input condition: >= MIN_CONDITION)"""
    x = np.asarray(x, dtype=np.float64)
    g = np.abs(spectrum(x, b))
    return float((g.min(axis=(2, 3)) / np.abs(x).sum(axis=(2, 3))).min())


@functools.lru_cache(maxsize=None)
def pick_seed(shape, b, start=0):
    """the first seed >= start whose content AND style meet the input condition"""
    for seed in range(start, start + 64):
        c, s = inputs(shape, seed)
        if condition(c, b) >= MIN_CONDITION and condition(s, b) >= MIN_CONDITION:
            return seed
    raise AssertionError(f"no seed in [{start}, {start + 64}) meets the input condition at {shape}, b = {b}")


def fft_form(content, style, b, alpha=1.0):
    c, s = np.asarray(content, dtype=np.float64), np.asarray(style, dtype=np.float64)
    H, W = c.shape[-2:]
    fc, fs = np.fft.fft2(c, axes=(-2, -1)), np.fft.fft2(s, axes=(-2, -1))
    ac, pc = np.abs(fc), np.angle(fc)
    a_c, a_s = np.fft.fftshift(ac, axes=(-2, -1)), np.fft.fftshift(np.abs(fs), axes=(-2, -1))
    ch, cw = H // 2, W // 2
    blk = (Ellipsis, slice(ch - b, ch + b + 1), slice(cw - b, cw + b + 1))
    a_c[blk] = (1.0 - alpha) * a_c[blk] + alpha * a_s[blk]
    a_new = np.fft.ifftshift(a_c, axes=(-2, -1))
    return np.real(np.fft.ifft2(a_new * np.exp(1j * pc), axes=(-2, -1)))


def _window_terms(gc, gs, H, W, b, mean, std):
    """(G_c', G_s', k): the coefficients the amplitudes and phases are formed on and the scale of dF - the raw-space DC variant touches [.., b, 0]"""
    gc, gs = gc.copy(), gs.copy()
    k = np.ones(gc.shape)
    if mean is not None:
        m, sd = np.asarray(mean, dtype=np.float64)[None, :], np.asarray(std, dtype=np.float64)[None, :]
        gc[:, :, b, 0] = sd * gc[:, :, b, 0] + m * H * W
        gs[:, :, b, 0] = sd * gs[:, :, b, 0] + m * H * W
        k[:, :, b, 0] = 1.0 / sd
    return gc, gs, k


def delta_f(gc, gs, H, W, b, alpha, mean=None, std=None):
    gc2, gs2, k = _window_terms(gc, gs, H, W, b, mean, std)
    ac, as_ = np.abs(gc2), np.abs(gs2)
    phase = np.where(ac == 0, 1.0 + 0j, gc2 / np.where(ac == 0, 1.0, ac))
    return k * alpha * (as_ - ac) * phase


def synthesis(df, H, W, b):
    """IDFT2 of the Hermitian extension of dF [N, C, 2b+1, b+1] -> real [N, C, H, W]"""
    eh = _twiddles(H, np.arange(-b, b + 1), +1.0)        # [2b+1, H]
    ew = _twiddles(W, np.arange(0, b + 1), +1.0)         # [b+1, W]
    S = np.matmul(eh.T, df)                              # [N, C, H, b+1]
    wgt = np.where(np.arange(b + 1) == 0, 1.0, 2.0)
    return np.real(np.matmul(S * wgt, ew)) / (H * W)


def low_rank(content, style, b, alpha=1.0, mean=None, std=None, clamp=None):
    c, s = np.asarray(content, dtype=np.float64), np.asarray(style, dtype=np.float64)
    H, W = c.shape[-2:]
    out = c + synthesis(delta_f(spectrum(c, b), spectrum(s, b), H, W, b, alpha, mean, std), H, W, b)
    if clamp is not None:
        lo, hi = (np.asarray(v, dtype=np.float64).reshape(1, -1, 1, 1) for v in clamp)
        out = np.maximum(np.minimum(out, hi), lo)
    return out


def raw_reference(content, style, b, alpha, mean, std):
    """normalise(FDA(denormalise(content), denormalise(style))) through the textbook pipeline"""
    m, sd = (np.asarray(v, dtype=np.float64).reshape(1, -1, 1, 1) for v in (mean, std))
    raw = fft_form(np.asarray(content, dtype=np.float64) * sd + m, np.asarray(style, dtype=np.float64) * sd + m, b, alpha)
    return (raw - m) / sd


def spectrum_bar(x, b):
    """E(G) per component, [N, C, 1, 1] (the same for every coefficient of a plane)"""
    x = np.asarray(x, dtype=np.float64)
    H, W = x.shape[-2:]
    return U32 * chain_spec(H, W) * np.abs(x).sum(axis=(2, 3))[:, :, None, None]


def transfer_bar(content, style, b, alpha, mean=None, std=None):
    """bar [N, C, H, W] of the transferred image before the clamp (a clamp only shrinks differences)"""
    c, s = np.asarray(content, dtype=np.float64), np.asarray(style, dtype=np.float64)
    H, W = c.shape[-2:]
    gc, gs = spectrum(c, b), spectrum(s, b)
    ec = np.broadcast_to(spectrum_bar(c, b), gc.shape).copy()
    es = np.broadcast_to(spectrum_bar(s, b), gs.shape).copy()
    gc2, gs2, k = _window_terms(gc, gs, H, W, b, mean, std)
    if mean is not None:
        m, sd = np.abs(np.asarray(mean, dtype=np.float64))[None, :], np.asarray(std, dtype=np.float64)[None, :]
        ec[:, :, b, 0] = sd * ec[:, :, b, 0] + 2 * U32 * (sd * np.abs(gc[:, :, b, 0]) + m * H * W)
        es[:, :, b, 0] = sd * es[:, :, b, 0] + 2 * U32 * (sd * np.abs(gs[:, :, b, 0]) + m * H * W)
    ac, as_ = np.abs(gc2), np.abs(gs2)
    rel = np.where(ec == 0, 0.0, ec / np.where(ac == 0, 1.0, ac))
    assert not np.any((ec > 0) & (ac == 0)), "a zero coefficient of a non-zero plane: the phase term has no bound"
    e_df = k * alpha * (es + ec + 2 * np.abs(as_ - ac) * rel + 6 * U32 * (as_ + ac))
    wgt = np.where(np.arange(b + 1) == 0, 1.0, 2.0)[None, None, None, :]
    mod = np.abs(delta_f(gc, gs, H, W, b, alpha, mean, std))
    abs_sum = (wgt * mod).sum(axis=(2, 3))[:, :, None, None] / (H * W)
    carried = (wgt * e_df).sum(axis=(2, 3))[:, :, None, None] / (H * W)
    return U32 * chain_out(b) * (np.abs(c) + abs_sum) + carried


def emulate_c64(content, style, b, alpha=1.0):
    """The low-rank chain in numpy float32 / complex64 (numpy's own summation order): what fp32 arithmetic gives without the kernels' layout.
    -> (spectrum of the content as complex64, transferred image as float32)"""
    c, s = np.asarray(content, dtype=np.float32), np.asarray(style, dtype=np.float32)
    H, W = c.shape[-2:]
    eh = _twiddles(H, np.arange(-b, b + 1), -1.0).astype(np.complex64)
    ew = _twiddles(W, np.arange(0, b + 1), -1.0).astype(np.complex64)
    gc = np.matmul(np.matmul(eh, c.astype(np.complex64)), ew.T)
    gs = np.matmul(np.matmul(eh, s.astype(np.complex64)), ew.T)
    ac, as_ = np.abs(gc), np.abs(gs)
    phase = np.where(ac == 0, np.complex64(1), gc / np.where(ac == 0, np.float32(1), ac))
    df = (np.float32(alpha) * (as_ - ac) * phase).astype(np.complex64)
    S = np.matmul(np.conj(eh).T, df)
    wgt = np.where(np.arange(b + 1) == 0, 1.0, 2.0).astype(np.complex64)
    img = np.real(np.matmul(S * wgt, np.conj(ew))).astype(np.float32) * np.float32(1.0 / (H * W))
    return gc, (c + img).astype(np.float32)
