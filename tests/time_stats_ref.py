"""Time statistics (include/gs_hip.h: gs_time_stats_*) restated in numpy, sample by sample, and as a literal per-cell
Python loop that the restatement is held to on small arrays.  Nothing here imports the library.

Every accumulator is compared by its bit pattern.  One freedom is left, and it is IEEE 754's, not a tolerance: the sign and
the payload of a NaN that an operation produces (inf - inf) or passes on are not specified, and x86 and gfx950 choose
differently -- so two NaNs are the same result whatever their bits (``same_bits``)."""
import numpy as np

SUM, SQUARES, EXTREMES, CROSSINGS = 1, 2, 4, 8
ALL = SUM | SQUARES | EXTREMES | CROSSINGS
NEVER = 0xFFFFFFFF
RAW_GROUP = {"sum": SUM, "squares": SQUARES, "min": EXTREMES, "max": EXTREMES, "set_count": CROSSINGS, "first_stamp": CROSSINGS}
RESULT_GROUPS = {"mean": SUM, "variance": SUM | SQUARES, "min": EXTREMES, "max": EXTREMES, "occupancy": CROSSINGS,
                 "arrival": CROSSINGS}
STAMPS = (3, 10, 11, 40, 41, 4000000000)


def raw_names(groups):
    return [name for name, g in RAW_GROUP.items() if groups & g]


def result_names(groups):
    return [name for name, g in RESULT_GROUPS.items() if groups & g == g]


def is_set(x, threshold, above):
    """The set rule of the thresholded observables: one f32 comparison; NaN and a cell equal to the threshold are unset."""
    t = np.float32(threshold)
    return x > t if above else x < t


class Accumulators:
    """The accumulators of one plane (any array shape), at their reset values."""

    def __init__(self, shape, groups=ALL, threshold=None, above=True):
        self.groups, self.threshold, self.above, self.samples = groups, threshold, above, 0
        self.sum = np.zeros(shape, np.float64)
        self.squares = np.zeros(shape, np.float64)
        self.min = np.full(shape, np.inf, np.float32)
        self.max = np.full(shape, -np.inf, np.float32)
        self.set_count = np.zeros(shape, np.uint32)
        self.first_stamp = np.full(shape, NEVER, np.uint32)

    def accumulate(self, x, stamp):
        """The table of gs_hip.h, in its order."""
        assert x.dtype == np.float32 and x.shape == self.sum.shape and 0 <= stamp < NEVER
        with np.errstate(all="ignore"):
            x64 = x.astype(np.float64)
            self.sum = self.sum + x64
            self.squares = self.squares + x64 * x64
            self.min = np.where(x < self.min, x, self.min)
            self.max = np.where(x > self.max, x, self.max)
            if self.threshold is not None:
                hit = is_set(x, self.threshold, self.above)
                self.set_count = self.set_count + hit.astype(np.uint32)
                self.first_stamp = np.where(hit & (self.first_stamp == NEVER), np.uint32(stamp), self.first_stamp)
        self.samples += 1

    def raw(self, name):
        return getattr(self, name)

    def result(self, name):
        """The result formulas in f64, every operation rounded once, one conversion to f32 at the end."""
        n = np.float64(self.samples)
        with np.errstate(all="ignore"):
            if name == "mean":
                return (self.sum / n).astype(np.float32)
            if name == "variance":
                m = self.sum / n
                d = self.squares / n - m * m
                return np.where(d <= 0.0, 0.0, d).astype(np.float32)        # (a NaN d stays NaN)
            if name in ("min", "max"):
                return self.raw(name)
            if name == "occupancy":
                return (self.set_count.astype(np.float64) / n).astype(np.float32)
            if name == "arrival":
                return np.where(self.first_stamp == NEVER, np.float32(-1.0), self.first_stamp.astype(np.float32))
        raise ValueError(name)


def literal(samples, stamps, threshold=None, above=True):
    """The same, cell by cell and sample by sample in plain Python over numpy scalars: {name: array} of the raw
    accumulators and, under "result:<name>", of the result planes."""
    shape = samples[0].shape
    acc = Accumulators(shape, ALL, threshold, above)
    raw = {name: acc.raw(name).copy() for name in RAW_GROUP}
    n = np.float64(len(samples))
    out = {"result:" + name: np.zeros(shape, np.float32) for name in RESULT_GROUPS}
    with np.errstate(all="ignore"):
        for idx in np.ndindex(*shape):
            s, q = np.float64(0.0), np.float64(0.0)
            mn, mx = np.float32(np.inf), np.float32(-np.inf)
            count, first = 0, NEVER
            for x_plane, stamp in zip(samples, stamps):
                x = np.float32(x_plane[idx])
                s = s + np.float64(x)
                q = q + np.float64(x) * np.float64(x)
                mn = x if x < mn else mn
                mx = x if x > mx else mx
                if threshold is not None:
                    hit = bool(x > np.float32(threshold)) if above else bool(x < np.float32(threshold))
                    if hit:
                        count += 1
                        if first == NEVER:
                            first = stamp
            raw["sum"][idx], raw["squares"][idx], raw["min"][idx], raw["max"][idx] = s, q, mn, mx
            raw["set_count"][idx], raw["first_stamp"][idx] = count, first
            m = s / n
            d = q / n - m * m
            out["result:mean"][idx] = np.float32(m)
            out["result:variance"][idx] = np.float32(d if d > 0 else (d if d != d else 0.0))
            out["result:min"][idx], out["result:max"][idx] = mn, mx
            out["result:occupancy"][idx] = np.float32(np.float64(count) / n)
            out["result:arrival"][idx] = np.float32(-1.0) if first == NEVER else np.float32(np.uint32(first))
    out.update(raw)
    return out


def same_bits(a, b):
    """Equal bit patterns cell for cell; two NaNs are the same result whatever their sign and payload."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    bits = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(np.all((a.view(bits) == b.view(bits)) | (np.isnan(a) & np.isnan(b))))


def describe(a, b):
    """Where two arrays differ, for an assertion's message."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return f"{a.dtype}{a.shape} against {b.dtype}{b.shape}"
    bad = a != b if a.dtype.kind != "f" else ~((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b)))
    where = np.argwhere(bad)
    if len(where) == 0:
        return "equal"
    i = tuple(where[0])
    return f"{len(where)} of {a.size} cells differ; first at {i}: {a[i]!r} against {b[i]!r}"


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-39, 3.4028235e38, -3.4028235e38],
                    np.float32)


def sample_planes(shape, seed, threshold, count=len(STAMPS)):
    """``count`` sample planes of ``shape`` that exercise every rule: by flat cell index i -- i % 4 == 0: a sequence that
    ascends from sample to sample, == 1: one that descends, == 2: zeros of alternating sign, else random values around the
    threshold --, then a tenth of the cells of every sample salted with the special values and with the threshold itself."""
    rng = np.random.default_rng(seed)
    size = int(np.prod(shape))
    kind = np.arange(size) % 4
    base = (rng.standard_normal(size) * 0.25 + threshold).astype(np.float32)
    step = np.abs(rng.standard_normal(size) * 0.1).astype(np.float32) + np.float32(1e-3)
    out = []
    for k in range(count):
        x = (rng.standard_normal(size) * 0.3 + threshold).astype(np.float32)
        x = np.where(kind == 0, base + np.float32(k) * step, x)
        x = np.where(kind == 1, base - np.float32(k) * step, x)
        x = np.where(kind == 2, np.float32(-0.0) if (k + seed) % 2 else np.float32(0.0), x).astype(np.float32)
        salted = rng.choice(size, size=(size + 9) // 10, replace=False)
        values = np.concatenate([SPECIALS, np.full(4, threshold, np.float32)])
        x[salted] = values[rng.integers(0, len(values), size=len(salted))]
        out.append(x.reshape(shape))
    return out
