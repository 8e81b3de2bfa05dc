"""A numpy restatement of the power spectrum's definition (include/gs_hip.h: gs_fields_spectrum), vectorised over tiles: the
same butterflies in the same order, every f32 operation rounded on its own (numpy's float32 ufuncs do that), the same f64
halving of the mean and the same fold.  The tables are arguments: the tests hand in the library's own
(``gs_spectrum_tables``), so that no last-bit difference between two libm's reaches a result."""
import numpy as np

TILES = (16, 32, 64, 128)
SEGMENT = 16  # tiles of a segment


def bit_reversal(T):
    bits = T.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(T)], np.int64)


def halve(p):
    """p[..., n] -> p[..., 0:n/2] + p[..., n/2:n], and so on down to one value."""
    while p.shape[-1] > 1:
        n = p.shape[-1] // 2
        p = p[..., :n] + p[..., n:]
    return p[..., 0]


def transform(re, im, wr, wi):
    """The radix-2 decimation-in-time transform of gs_hip.h along the last axis of the f32 arrays (re, im)."""
    T = re.shape[-1]
    order = bit_reversal(T)
    re, im = np.ascontiguousarray(re[..., order]), np.ascontiguousarray(im[..., order])
    lead = re.shape[:-1]
    h = 1
    while h < T:
        shape = lead + (T // (2 * h), 2, h)
        r, i = re.reshape(shape), im.reshape(shape)
        a_re, a_im, b_re, b_im = r[..., 0, :], i[..., 0, :], r[..., 1, :], i[..., 1, :]
        k = np.arange(h) * (T // (2 * h))
        w_re, w_im = wr[k], wi[k]
        t_re = b_re * w_re - b_im * w_im
        t_im = b_re * w_im + b_im * w_re
        re = np.stack([a_re + t_re, a_re - t_re], axis=-2).reshape(lead + (T,))
        im = np.stack([a_im + t_im, a_im - t_im], axis=-2).reshape(lead + (T,))
        h *= 2
    return re, im


def tile_mean(tiles):
    """m of gs_hip.h for f32 tiles [n, T, T]: f32 [n]."""
    T = tiles.shape[-1]
    total = halve(halve(tiles.astype(np.float64)))
    return (total / float(T * T)).astype(np.float32)


def tile_power(tiles, h, w, window):
    """p[n, T, T/2 + 1] (f32) of f32 tiles [n, T, T] that hold only finite cells; h: f32 [T], w: complex64 [T/2]."""
    tiles = np.asarray(tiles, np.float32)
    T = tiles.shape[-1]
    h = np.asarray(h, np.float32)
    wr, wi = np.ascontiguousarray(w.real, np.float32), np.ascontiguousarray(w.imag, np.float32)
    assert wr.dtype == np.float32 and tiles.dtype == np.float32
    with np.errstate(all="ignore"):
        y = tiles - tile_mean(tiles)[:, None, None]
        if window:
            y = (y * h[None, :, None]) * h[None, None, :]
        re, im = transform(y, np.zeros_like(y), wr, wi)                  # rows: [n, r, kc]
        re, im = re[..., :T // 2 + 1], im[..., :T // 2 + 1]
        re, im = transform(re.transpose(0, 2, 1), im.transpose(0, 2, 1), wr, wi)  # columns: [n, kc, kr]
        re, im = re.transpose(0, 2, 1), im.transpose(0, 2, 1)
        p = re * re + im * im
    assert p.dtype == np.float32
    return p


def tiles_of(x, T):
    """The whole tiles of the plane x as [bands, tiles per band, T, T]."""
    x = np.asarray(x, np.float32)
    nb, nt = x.shape[0] // T, x.shape[1] // T
    return x[:nb * T, :nt * T].reshape(nb, T, nt, T).transpose(0, 2, 1, 3)


def spectrum(x, T, window, h, w):
    """(power f64 [T, T/2 + 1], tiles uint64 [2] = {used, skipped}) of the plane x."""
    t = tiles_of(x, T)
    nb, nt = t.shape[:2]
    power = np.zeros((T, T // 2 + 1), np.float64)
    counts = np.zeros(2, np.uint64)
    if nb == 0 or nt == 0:
        return power, counts
    flat = t.reshape(nb * nt, T, T)
    finite = np.isfinite(flat).all(axis=(1, 2))
    p = np.zeros((nb * nt, T, T // 2 + 1), np.float64)
    if finite.any():
        p[finite] = tile_power(flat[finite], h, w, window).astype(np.float64)
    with np.errstate(all="ignore"):
        for b in range(nb):
            band = np.zeros_like(power)
            for s0 in range(0, nt, SEGMENT):
                record = np.zeros_like(power)
                for j in range(s0, min(s0 + SEGMENT, nt)):
                    if finite[b * nt + j]:
                        record = record + p[b * nt + j]
                band = band + record
            power = power + band
    counts[0] = int(finite.sum())
    counts[1] = int((~finite).sum())
    return power, counts


def exact_power(tiles, h, window):
    """|rfft2|^2 in f64 of f32 tiles [n, T, T] after the same mean (the f32 value m) and window (the f32 table) applied in
    f64: what tile_power approximates."""
    tiles = np.asarray(tiles, np.float32)
    y = tiles.astype(np.float64) - tile_mean(tiles).astype(np.float64)[:, None, None]
    if window:
        h64 = np.asarray(h, np.float32).astype(np.float64)
        y = (y * h64[None, :, None]) * h64[None, None, :]
    return np.abs(np.fft.rfft2(y, axes=(1, 2))) ** 2


def bound(T):
    """B(T): sum |p - P| <= B(T) sum P for one tile (the issue's error analysis of log2 T stages per axis in f32)."""
    u = 2.0 ** -24
    gamma = 4 * u / (1 - 4 * u)
    eta = u + gamma * (np.sqrt(2.0) + u)
    L = 2 * (T.bit_length() - 1)
    c = L * eta / (1 - L * eta)
    delta = c + 3 * u * (1 + c)
    return 2 * delta + delta ** 2 + 2 * u * (1 + delta) ** 2
