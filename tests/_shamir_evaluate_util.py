"""Shared by the share-repair tests: the contract restated in Python integers on top of the exhaustive search of
_shamir_correct_util (imported as it is), and the target mixes the tests walk."""
from _shamir_correct_util import UNDECODABLE, _basis_weights, _interpolate, restated


def restated_values(indices, rows, t, p, targets):
    """(values, (out, nerr, col_err, masks)): the search finds each row's polynomial and the columns off it; the polynomial is the
    one through t + 1 of the other columns, evaluated at every target's point.  An undecodable row is all 0."""
    report = restated(indices, rows, t, p)
    xs = [i + 1 for i in indices]
    values = []
    for row, n, mk in zip(rows, report[1], report[3]):
        if n == UNDECODABLE:
            values.append([0] * len(targets))
            continue
        basis = [c for c in range(len(xs)) if not (mk >> c) & 1][:t + 1]
        assert len(basis) == t + 1
        bx, by = [xs[c] for c in basis], [row[c] % p for c in basis]
        w = _basis_weights(bx, p)
        values.append([_interpolate(bx, by, w, tg + 1, p) for tg in targets])
    return values, report


def off_points(indices, p, how_many, rng):
    """party indices below p - 1 that are none of `indices`: small ones, one next to the top where there is room"""
    taken, out = set(indices), []
    if p - 2 not in taken:
        out.append(p - 2)
    while len(out) < how_many:
        v = rng.randrange(min(p - 1, 1 << 20))
        if v not in taken and v not in out:
            out.append(v)
    return out[:how_many]


def target_mixes(indices, wrong, p, rng):
    """name -> targets: none of the points (T = 1, 2 and 7), all columns in order, only the columns in `wrong`, only columns that
    are not, duplicates, and a shuffled mix of 7"""
    count = len(indices)
    right = [c for c in range(count) if c not in wrong]
    room = p - 1 - count                                  # indices that are no column
    mixes = {"columns": list(indices)}
    for T in (1, 2, 7):
        if room >= T:
            mixes[f"off{T}"] = off_points(indices, p, T, rng)
    if wrong:
        mixes["wrong"] = [indices[c] for c in sorted(wrong)]
    if right:
        mixes["right"] = [indices[c] for c in right]
    a = indices[rng.randrange(count)]
    b = off_points(indices, p, 1, rng)[0] if room >= 1 else indices[0]
    mixes["duplicates"] = [a, b, a, a, b]
    mixed = [indices[rng.randrange(count)] for _ in range(4)] + (off_points(indices, p, 3, rng) if room >= 3 else [indices[0]] * 3)
    rng.shuffle(mixed)
    mixes["mixed7"] = mixed
    return mixes
