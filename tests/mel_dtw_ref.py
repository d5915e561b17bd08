"""float64 restatement of tts_hip_mel_dtw (include/tts_hip.h): every stage, the path and the statistics, for one pair.

`dtype=np.float32` runs the same statements in float32 (the "float32 numpy copy" the CPU test holds the GPU bounds above);
`mistake=` plants one of MISTAKES, which the CPU test holds a factor ten above the bounds.  The bounds themselves are here
too, so that the CPU and the GPU test assert the same ones.
"""
import numpy as np

EPS = 2.0 ** -24                                                  # half an ulp of float32, relative
MCD_DB_FACTOR = 10.0 * np.sqrt(2.0) / np.log(10.0)
STAGES = ('cepstra_a', 'cepstra_b', 'distance', 'cost', 'step')
MISTAKES = ('c0 kept', 'dct without the half sample', 'one coefficient short', 'sqrt missing', 'no diagonal step',
            'diagonal counted twice', 'pad frames included', 'last frame dropped', 'ln instead of log10')


def dct_table(n_mel, n_cep, c0=False, rounded=True, half=0.5):
    """[R, n_mel] float64: rows 1 .. n_cep (0 .. n_cep with c0) of the orthonormal DCT-II; `rounded`: through float32 once, as
    the engine keeps it."""
    r = np.arange(0 if c0 else 1, n_cep + 1, dtype=np.float64)[:, None]
    k = np.arange(n_mel, dtype=np.float64)[None]
    D = np.sqrt(2.0 / n_mel) * np.cos(np.pi * (k + half) * r / n_mel)
    D = np.where(r == 0, D / np.sqrt(2.0), D)
    return D.astype(np.float32).astype(np.float64) if rounded else D


def cepstra(m, D, dtype=np.float64):
    """m [T, n_mel] -> [T, R]; every frame by the same sequence of operations (equal frames give equal cepstra, bit for bit)"""
    return (np.asarray(m, dtype)[:, None, :] * np.asarray(D, dtype)[None]).sum(axis=-1, dtype=dtype)


def cepstra_bound(m, D):
    """[T, R]: (n_mel + 1) 2^-24 sum_k |D[r][k] m[k]|"""
    return (D.shape[1] + 1) * EPS * (np.abs(np.asarray(m, np.float64)) @ np.abs(D).T)


def distance(ca, cb, dtype=np.float64, sqrt=True):
    """[la, R], [lb, R] -> d [la, lb]"""
    diff = np.asarray(ca, dtype)[:, None, :] - np.asarray(cb, dtype)[None, :, :]
    s = (diff * diff).sum(axis=-1, dtype=dtype)
    return np.sqrt(s) if sqrt else s


def accumulate(d, dtype=np.float64, diagonal=True, diagonal_weight=1):
    """d [la, lb] -> (C [la, lb], step [la, lb] int): the recursion of the header, anti-diagonal by anti-diagonal; ties
    resolve diagonal, (i-1, j), (i, j-1)."""
    d = np.asarray(d, dtype)
    la, lb = d.shape
    Cp = np.full((la + 1, lb + 1), np.inf, dtype)                 # Cp[i + 1, j + 1] = C(i, j)
    Cp[0, 0] = 0                                                  # stands before (0, 0): C(0, 0) = d(0, 0) + 0, exactly d(0, 0)
    step = np.zeros((la, lb), np.int64)
    for k in range(la + lb - 1):
        i = np.arange(max(0, k - lb + 1), min(la - 1, k) + 1)
        j = k - i
        dg, up, left = Cp[i, j], Cp[i, j + 1], Cp[i + 1, j]
        dd = d[i, j]
        code = np.zeros(len(i), np.int64)
        if diagonal and diagonal_weight == 1:                     # the definition: min over the neighbours, then one add
            best = dg
            m = up < best
            best, code = np.where(m, up, best), np.where(m, 1, code)
            m = left < best
            best, code = np.where(m, left, best), np.where(m, 2, code)
            new = dd + best
        else:                                                     # the planted step patterns: min over the weighted sums
            new = dd * dtype(diagonal_weight) + dg if diagonal and k > 0 else np.full(len(i), np.inf, dtype)
            for c, other in ((1, dd + up), (2, dd + left)):
                m = other < new
                new, code = np.where(m, other, new), np.where(m, c, code)
            if k == 0:
                new = dd.copy()
        Cp[i + 1, j + 1] = new
        step[i, j] = code
    return Cp[1:, 1:].copy(), step


def argmin_codes(C):
    """The documented step code of every cell of a given cost matrix (missing neighbours = +inf; cell (0, 0): 0)."""
    C = np.asarray(C)
    la, lb = C.shape
    Cp = np.full((la + 1, lb + 1), np.inf, C.dtype)
    Cp[1:, 1:] = C
    dg, up, left = Cp[:-1, :-1], Cp[:-1, 1:], Cp[1:, :-1]
    code = np.zeros((la, lb), np.int64)
    best = dg.copy()
    m = up < best
    best, code = np.where(m, up, best), np.where(m, 1, code)
    m = left < best
    return np.where(m, 2, code)


def backtrack(step):
    """step [la, lb] -> the path [(i, j)] from (0, 0) to (la - 1, lb - 1)."""
    i, j = step.shape[0] - 1, step.shape[1] - 1
    path = [(i, j)]
    while (i, j) != (0, 0):
        code = 2 if i == 0 else 1 if j == 0 else int(step[i, j])
        i, j = i - (code != 2), j - (code != 1)
        path.append((i, j))
    return path[::-1]


def margin_along(C, path):
    """The smallest gap between the best and the second-best predecessor over the cells of `path` (inf where only one exists)."""
    la, lb = C.shape
    Cp = np.full((la + 1, lb + 1), np.inf)
    Cp[1:, 1:] = C
    gap = np.inf
    for i, j in path[1:]:
        v = sorted((Cp[i, j], Cp[i, j + 1], Cp[i + 1, j]))
        gap = min(gap, v[1] - v[0])
    return gap


def cost_bound(n_cep, la, lb, cost):
    """End to end, from the run's own cepstra: (n_cep + 4 + la + lb) 2^-24 cost"""
    return (n_cep + 4 + la + lb) * EPS * cost


def mel_dtw(a, b, la=None, lb=None, n_cep=13, c0=False, align=True, dtype=np.float64, mistake=None, cepstra_in=None):
    """One pair: a [Ta, n_mel], b [Tb, n_mel] with la / lb real frames -> dict(cepstra_a, cepstra_b, distance, cost (the matrix),
    step, path, stats = (cost, path_len, mcd)).  `cepstra_in` = (ca, cb): start from these instead of the mels."""
    assert mistake is None or mistake in MISTAKES, mistake
    a, b = np.asarray(a), np.asarray(b)
    la, lb = a.shape[0] if la is None else int(la), b.shape[0] if lb is None else int(lb)
    if mistake == 'pad frames included':
        la, lb = a.shape[0], b.shape[0]
    if mistake == 'last frame dropped':
        la, lb = max(la - 1, 1), max(lb - 1, 1)
    D = dct_table(a.shape[1], n_cep - (mistake == 'one coefficient short'), c0 or mistake == 'c0 kept',
                  half=0.0 if mistake == 'dct without the half sample' else 0.5)
    if cepstra_in is None:
        ca, cb = cepstra(a[:la], D, dtype), cepstra(b[:lb], D, dtype)
    else:
        ca, cb = (np.asarray(x, dtype) for x in cepstra_in)
    d = distance(ca, cb, dtype, sqrt=mistake != 'sqrt missing')
    out = dict(cepstra_a=ca, cepstra_b=cb, distance=d)
    if align:
        C, step = accumulate(d, dtype, diagonal=mistake != 'no diagonal step',
                             diagonal_weight=2 if mistake == 'diagonal counted twice' else 1)
        path = backtrack(step)
        cost = C[-1, -1]
        out.update(cost=C, step=step)
    else:
        n = min(la, lb)
        path = [(t, t) for t in range(n)]
        cost = d[np.arange(n), np.arange(n)].sum(dtype=np.float64)
    factor = 10.0 * np.sqrt(2.0) if mistake == 'ln instead of log10' else MCD_DB_FACTOR
    out.update(path=path, stats=np.array([cost, len(path), factor * float(cost) / len(path)], np.float64))
    return out


def enumerate_optimum(d):
    """The minimum over every monotone path from (0, 0) to (la - 1, lb - 1) of the sum of d along it, by enumeration."""
    la, lb = d.shape

    def walk(i, j):
        if (i, j) == (la - 1, lb - 1):
            return d[i, j]
        nxt = [walk(i + di, j + dj) for di, dj in ((1, 1), (1, 0), (0, 1)) if i + di < la and j + dj < lb]
        return d[i, j] + min(nxt)

    return walk(0, 0)
