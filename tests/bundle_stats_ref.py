"""Bundle statistics (include/gs_hip.h: gs_members_bundle_stats) restated in numpy -- a loop over a bundle's members in
ascending order, vectorised over cells, f64 exactly as defined -- and as a literal per-cell, per-member Python loop that the
restatement is held to on tiny grids.  Nothing here imports the library.

Results are compared by bit pattern with ``time_stats_ref.same_bits``: the sign and payload of a NaN are IEEE 754's freedom."""
import numpy as np

from tests.time_stats_ref import describe, same_bits  # noqa: F401  (re-exported for the tests)

RESULTS = ("mean", "variance", "min", "max", "occupancy")
CODES = {"mean": 0, "variance": 1, "min": 2, "max": 3, "occupancy": 4}   # GS_TSTAT_MEAN .. GS_TSTAT_OCCUPANCY


def is_set(x, threshold, above):
    """Morphology's rule: one f32 comparison; NaN and a cell equal to the threshold are unset."""
    t = np.float32(threshold)
    return x > t if above else x < t


def bundle(members, threshold=None, above=True):
    """{name: plane} of ONE bundle of one species: ``members`` is ``[span, ...]`` f32, visited in ascending order."""
    members = np.asarray(members)
    assert members.dtype == np.float32 and members.shape[0] >= 1
    shape = members.shape[1:]
    s, q = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    mn, mx = np.full(shape, np.inf, np.float32), np.full(shape, -np.inf, np.float32)
    count = np.zeros(shape, np.uint32)
    with np.errstate(all="ignore"):
        for x in members:
            x64 = x.astype(np.float64)
            s = s + x64
            q = q + x64 * x64
            mn = np.where(x < mn, x, mn)
            mx = np.where(x > mx, x, mx)
            if threshold is not None:
                count = count + is_set(x, threshold, above).astype(np.uint32)
        n = np.float64(members.shape[0])
        m = s / n
        d = q / n - m * m
        out = {"mean": m.astype(np.float32), "variance": np.where(d <= 0.0, 0.0, d).astype(np.float32),   # (a NaN d stays NaN)
               "min": mn, "max": mx}
        if threshold is not None:
            out["occupancy"] = (count.astype(np.float64) / n).astype(np.float32)
    return out


def bundles(planes, span, threshold=None, above=True):
    """{name: [count / span, ...]} of the bundles of ``planes`` = ``[count, ...]`` of one species."""
    planes = np.asarray(planes)
    assert span >= 1 and planes.shape[0] % span == 0
    each = [bundle(planes[b * span:(b + 1) * span], threshold, above) for b in range(planes.shape[0] // span)]
    names = each[0].keys() if each else ()
    return {name: np.stack([e[name] for e in each]) for name in names}


def literal(members, threshold=None, above=True):
    """The same bundle cell by cell and member by member in plain Python over numpy scalars."""
    members = np.asarray(members)
    shape = members.shape[1:]
    n = np.float64(members.shape[0])
    out = {name: np.zeros(shape, np.float32) for name in RESULTS if name != "occupancy" or threshold is not None}
    with np.errstate(all="ignore"):
        for idx in np.ndindex(*shape):
            s, q = np.float64(0.0), np.float64(0.0)
            mn, mx = np.float32(np.inf), np.float32(-np.inf)
            count = 0
            for j in range(members.shape[0]):
                x = np.float32(members[(j,) + idx])
                s = s + np.float64(x)
                q = q + np.float64(x) * np.float64(x)
                mn = x if x < mn else mn
                mx = x if x > mx else mx
                if threshold is not None:
                    count += int(bool(x > np.float32(threshold)) if above else bool(x < np.float32(threshold)))
            m = s / n
            d = q / n - m * m
            out["mean"][idx] = np.float32(m)
            out["variance"][idx] = np.float32(d if d > 0 else (d if d != d else 0.0))
            out["min"][idx], out["max"][idx] = mn, mx
            if threshold is not None:
                out["occupancy"][idx] = np.float32(np.float64(count) / n)
    return out


SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-39, 3.4028235e38, -3.4028235e38],
                    np.float32)


def plant(planes, span, seed, threshold):
    """Plants the special values into ``planes`` = ``[count, rows, cols]`` (in place; returns it): for every bundle, the
    first, a middle and the last member each carry the bundle's largest and smallest value somewhere, and cells of chosen
    members get NaN, +-inf, sub-normals, the threshold itself and -0 / +0 pairs in both orders."""
    rng = np.random.default_rng(seed)
    count = planes.shape[0]
    flat = planes.reshape(count, -1)
    cells = flat.shape[1]
    for b in range(count // span):
        mem = sorted({b * span, b * span + span // 2, b * span + span - 1})
        picks = rng.choice(cells, size=min(cells, 2 * len(mem) + 6), replace=False)
        for k, m in enumerate(mem):                       # the extreme of a cell sits in the first / a middle / the last member
            flat[m, picks[2 * k]] = np.float32(7.0 + b)
            flat[m, picks[2 * k + 1]] = np.float32(-7.0 - b)
        rest = picks[2 * len(mem):]
        for k, c in enumerate(rest[:4]):                  # specials in chosen members
            flat[mem[k % len(mem)], c] = SPECIALS[(k + b + seed) % len(SPECIALS)]
        flat[b * span:(b + 1) * span, rest[4]] = np.float32(0.0)     # a cell of zeros: -0 first or last, +0 elsewhere
        flat[mem[0] if (b + seed) % 2 else mem[-1], rest[4]] = np.float32(-0.0)
        flat[mem[-1], rest[5]] = np.float32(threshold)    # equal to the threshold: not set
    salted = rng.choice(flat.size, size=(flat.size + 19) // 20, replace=False)
    values = np.concatenate([SPECIALS, np.full(3, threshold, np.float32)])
    flat.reshape(-1)[salted] = values[rng.integers(0, len(values), size=len(salted))]
    return planes
