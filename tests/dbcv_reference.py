"""The numpy f64 restatement of DBCV as include/dic_hip.h defines it -- the yardstick of test_dbcv_host.py and test_gpu_dbcv.py.  It shares no code with
dbcv.py: a dense distance matrix, the loop of Prim's walk with the walk's tie rule, and the rules for internal nodes and edges, written out again."""
import numpy as np


SIZES = (300, 250, 97, 3, 2, 1)          # clusters 0 .. 5 of ``blobs``: three that fill tiles raggedly, a path of three, a pair and a singleton
N_NOISE = 47
GRID = 2.0 ** -10


def blobs(D, seed=0):
    """``(X (700, D) f32, labels (700,) int64)``, shuffled: Gaussian blobs of ``SIZES`` members with sigma = 0.5 around centres 3 N(0, 1) per coordinate
    (about six sigma apart per coordinate) and ``N_NOISE`` noise rows uniform in [-10, 10]; rows 0 and 1 of cluster 0 coincide.
    EVERY COORDINATE IS A MULTIPLE OF 2^-10 BELOW 32 IN SIZE.  Then a difference is a multiple of 2^-10 below 64, its square a multiple of 2^-20 below
    2^12, and a sum of up to 256 of them a multiple of 2^-20 below 2^20: 40 bits.  Every d^2 is exact in f64 in whatever order it is summed, so the kernels,
    the walk and this yardstick hold the same bits for it, sqrt is correctly rounded on both sides, and discrete results (trees, internal nodes, arg-minima)
    and every value that is a maximum of ``a`` and distances can be compared exactly."""
    rng = np.random.RandomState(seed)
    parts, labels = [], []
    for c, n in enumerate(SIZES):
        centre = np.clip(3.0 * rng.randn(D), -12, 12)
        parts.append(centre + np.clip(0.5 * rng.randn(n, D), -4, 4))
        labels += [c] * n
    parts.append(rng.uniform(-10, 10, size=(N_NOISE, D)))
    labels += [-1] * N_NOISE
    X = np.round(np.concatenate(parts) / GRID) * GRID
    X[1] = X[0]
    labels = np.array(labels, dtype=np.int64)
    order = rng.permutation(len(X))
    X = X[order].astype(np.float32)
    assert np.abs(X).max() < 32 and np.array_equal(np.round(X.astype(np.float64) / GRID) * GRID, X)
    return X, labels[order]


def split_at_random(labels, cluster, new_id, seed=1):
    """``labels`` with a random half of ``cluster`` relabelled ``new_id``."""
    out = np.array(labels)
    rows = np.flatnonzero(out == cluster)
    out[np.random.RandomState(seed).permutation(rows)[:len(rows) // 2]] = new_id
    return out


def dmat(X):
    """(N, N) f64: the difference-form distances of the f32 coordinates, in row blocks (the differences of two f32 are exact in f64)."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    out = np.empty((len(X), len(X)))
    for s in range(0, len(X), 64):
        diff = X[s:s + 64, None, :] - X[None, :, :]
        out[s:s + 64] = np.sqrt((diff * diff).sum(-1))
    return out


def core_distances(D, d):
    """a(o) for the members of ONE cluster from their (n, n) distance matrix: over the members p with D[o, p] > 0."""
    n = len(D)
    a = np.zeros(n)
    for o in range(n):
        far = D[o][D[o] > 0]
        if far.size:
            m = far.min()
            S = np.exp(0.5 * d * np.log(m * m / (far * far))).sum()
            a[o] = m * (S / (n - 1)) ** (-1.0 / d)
    return a


def prim(W):
    """Prim from member 0 over the (n, n) weights: strict updates, the next point is the first minimum outside the tree.  ``(reach, pred)``."""
    n = len(W)
    reach, pred = np.full(n, np.inf), np.full(n, -1, dtype=np.int64)
    inside = np.zeros(n, dtype=bool)
    cur = 0
    for _ in range(n - 1):
        inside[cur] = True
        better = ~inside & (W[cur] < reach)
        reach[better], pred[better] = W[cur][better], cur
        cur = int(np.argmin(np.where(inside, np.inf, reach)))
    return reach, pred


def tree_rules(reach, pred):
    """``(DSC, internal)``: degree >= 2, else the first member; edges with both ends internal, else all edges; the largest such weight."""
    n = len(pred)
    deg = np.zeros(n, dtype=np.int64)
    for q in range(n):
        if pred[q] >= 0:
            deg[q] += 1
            deg[pred[q]] += 1
    internal = deg >= 2
    if not internal.any():
        internal[0] = True
    edges = [q for q in range(n) if pred[q] >= 0]
    inner = [q for q in edges if internal[q] and internal[pred[q]]]
    return max(reach[q] for q in (inner or edges)), internal


def reference(X, labels, d=None, a=None, D=None):
    """The definition on the dense matrix.  ``a``: per-row core distances to use instead of the oracle's own (the rows of kept clusters are read).  A dict
    with the fields of ``dbcv.DBCV``."""
    X, labels = np.asarray(X), np.asarray(labels).astype(np.int64)
    N = len(labels)
    d = X.shape[1] if d is None else d
    D = dmat(X) if D is None else D
    ids, counts = np.unique(labels, return_counts=True)
    kept = [int(c) for c, k in zip(ids, counts) if c != -1 and k >= 2]
    if len(kept) < 2:
        raise ValueError('fewer than two clusters')
    members = {c: np.flatnonzero(labels == c) for c in kept}
    core = np.full(N, np.nan)
    internal = np.zeros(N, dtype=bool)
    dsc = []
    for c in kept:
        rows = members[c]
        Dc = D[np.ix_(rows, rows)]
        core[rows] = core_distances(Dc, d) if a is None else np.asarray(a)[rows]
        ac = core[rows]
        reach, pred = prim(np.maximum(np.maximum(ac[:, None], ac[None, :]), Dc))
        s, inner = tree_rules(reach, pred)
        dsc.append(s)
        internal[rows] = inner
    sep, nearest = [], []
    for c in kept:
        mine = members[c][internal[members[c]]]
        other = np.concatenate([members[o][internal[members[o]]] for o in kept if o != c])          # (cluster, row) order
        M = np.maximum(np.maximum(core[mine][:, None], core[other][None, :]), D[np.ix_(mine, other)])
        at = int(np.argmin(M))          # the first minimum: the smallest o, then the smallest p
        sep.append(M.flat[at])
        nearest.append(labels[other[at % len(other)]])
    dsc, sep = np.array(dsc), np.array(sep)
    top = np.maximum(dsc, sep)
    validity = np.array([(s - c) / t if t > 0 else 0.0 for s, c, t in zip(sep, dsc, top)])
    sizes = np.array([len(members[c]) for c in kept])
    return dict(score=float((sizes / N * validity).sum()), cluster_ids=np.array(kept), sizes=sizes, sparseness=dsc, separation=sep, validity=validity,
                nearest_cluster=np.array(nearest), n_noise=int((labels == -1).sum()), n_singletons=int(((ids != -1) & (counts == 1)).sum()),
                core_distances_=core, internal_=internal)
