"""Shared by the corrected-reconstruction tests: sharings, planted errors, and the contract restated in Python
integers by exhaustive search (every polynomial through t + 1 of the columns is tried, so count stays small)."""
import itertools

U64 = (1 << 64) - 1
P61 = (1 << 61) - 1
P62 = (1 << 62) - 57
UNDECODABLE = 0xFFFFFFFF


def indices_for(count, p, rng):
    """distinct, unsorted, non-contiguous; one near 2^40 where p allows it"""
    top = p - 1
    idx = set()
    if top > (1 << 41):
        idx.add((1 << 40) - 3)
    while len(idx) < count:
        idx.add(rng.randrange(min(top, 1 << 20) if top > 300 else top))
    idx = list(idx)
    rng.shuffle(idx)
    return idx


def sharing(indices, t, p, S, rng):
    """S polynomials of degree t and their values at the points: (secrets, rows [S][count])"""
    polys = [[rng.randrange(p) for _ in range(t + 1)] for _ in range(S)]
    rows = [[sum(a[j] * pow(i + 1, j, p) for j in range(t + 1)) % p for i in indices] for a in polys]
    return [a[0] for a in polys], rows


def bend(rows, s, cols, p, rng):
    """a nonzero amount added to row s in every column of cols"""
    for c in cols:
        rows[s][c] = (rows[s][c] + 1 + rng.randrange(p - 1)) % p


def unreduce(rows, p, rng):
    """the same residues as words that are not below p, where they fit"""
    return [[v + p if rng.random() < 0.5 and v + p <= U64 else v for v in row] for row in rows]


def _basis_weights(bx, p):
    """1 / prod_{i != j}(x_j - x_i) for every basis point"""
    w = []
    for j, xj in enumerate(bx):
        den = 1
        for i, xi in enumerate(bx):
            if i != j:
                den = den * (xj - xi) % p
        w.append(pow(den, p - 2, p))
    return w


def _interpolate(bx, by, w, x, p):
    total = 0
    for j in range(len(bx)):
        num = 1
        for i in range(len(bx)):
            if i != j:
                num = num * (x - bx[i]) % p
        total += by[j] * num * w[j]
    return total % p


def restated(indices, rows, t, p):
    """(out, nerr, col_err, masks) by the contract: the nearest polynomial of degree <= t, if it is within E columns.  masks[s] is
    one Python integer, bit c for column c."""
    xs = [i + 1 for i in indices]
    count = len(xs)
    E = (count - t - 1) // 2
    out, nerr, col_err, masks = [], [], [0] * count, []
    weights = {}                                         # per basis, shared by the rows
    for row in rows:
        ys = [v % p for v in row]
        found = None
        for basis in itertools.combinations(range(count), t + 1):
            bx, by = [xs[c] for c in basis], [ys[c] for c in basis]
            w = weights.get(basis)
            if w is None:
                w = weights[basis] = _basis_weights(bx, p)
            off = []
            for c in range(count):
                if c not in basis and _interpolate(bx, by, w, xs[c], p) != ys[c]:
                    off.append(c)
                    if len(off) > E:
                        break
            if len(off) <= E:
                found = (_interpolate(bx, by, w, 0, p), off)
                break                                    # unique: two such polynomials would agree in >= t + 1 columns
        if found is None:
            out.append(0), nerr.append(UNDECODABLE), masks.append(0)
        else:
            out.append(found[0]), nerr.append(len(found[1])), masks.append(sum(1 << c for c in found[1]))
            for c in found[1]:
                col_err[c] += 1
    return out, nerr, col_err, masks


def mask_ints(err_mask):
    """[S][words] uint64 -> one Python integer per secret"""
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) for row in err_mask]
