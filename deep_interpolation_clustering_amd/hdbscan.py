"""HDBSCAN on the MI355X without the distance matrix (``sklearn.cluster.HDBSCAN``, euclidean).

HDBSCAN builds the hierarchy of all DBSCAN clusterings at once and keeps the clusters that persist, which spares the ``eps`` DBSCAN wants read off the
k-distance elbow and the ``xi`` OPTICS wants.  Its expensive part is Prim's minimum spanning tree of the mutual-reachability graph,
``mr(p, q) = max(core[p], core[q], d(p, q))``: N - 1 strictly sequential steps of O(N) each, on a CPU either on top of an N x N matrix (45 GB in f64 at
75 000 points) or with N^2 scalar distance calls.  Here the core distances come from ``knn.kth_neighbor_distance`` and every step of Prim's walk is one row
pass over the points on the device (csrc/dic_hdbscan.hip): the distances of the current point are recomputed, reachability and predecessor updated, and the
next point found, in one launch; the N - 1 launches are enqueued back to back and the host reads the result once.

The definition is sklearn's (1.7.2) in its self-consistent form -- ``HDBSCAN(metric='precomputed', algorithm='brute').fit(D)`` with ``D`` the f64
difference-form distances of the f32 points: one distance function serves the core distances and the steps (bit for bit, and symmetric), so the many ties of a
mutual-reachability tree (every edge into a sparse point weighs exactly that point's core distance) are broken by index, as sklearn's ``argmin`` breaks them.

ONE POINT IS FIXED HERE THAT sklearn LEAVES OPEN.  sklearn sorts the tree's edges by weight with ``np.argsort`` of the default kind, which is not stable, and
the union-find that follows depends on the order of equal weights: its labels depend on how numpy's sort happens to break ties (DESIGN.md section 5 has the
measurements).  This module sorts with a STABLE sort: equal weights stay in the order Prim's walk found them.  Where sklearn's own functions give the same
labels under both sort kinds, these are sklearn's labels.

Everything after the tree (``single_linkage_tree``, ``condense_tree``, ``tree_to_labels``, ``labelling_at_cut``) is O(N log N) host work in numpy and plain
loops and restates sklearn's ``_linkage.pyx`` / ``_tree.pyx`` operation for operation, so that probabilities agree to the last bit; sklearn itself is not
imported by the package.
"""
from __future__ import annotations

import numbers

import numpy as np

from . import knn
from .dbscan import MAX_DIM, _device_points
from .optics import device_walk

HIERARCHY_dtype = np.dtype([('left_node', np.intp), ('right_node', np.intp), ('value', np.float64), ('cluster_size', np.intp)])
CONDENSED_dtype = np.dtype([('parent', np.intp), ('child', np.intp), ('value', np.float64), ('cluster_size', np.intp)])
NOISE = -1


def hdbscan_mst(X, min_samples, stats=None):
    """Prim's walk over the mutual-reachability graph from point 0: ``(ordering int64, core f64, reach f64, pred int64)``, numpy, each (N,).  ``core`` is the
    unrounded distance to the ``min_samples``-th neighbour (the point itself counted), ``reach[q]`` the weight at which q joined the tree (inf for point 0),
    ``pred[q]`` its neighbour in the tree (-1 for point 0).  sklearn's edge record of step i is ``(ordering[i], ordering[i + 1], reach[ordering[i + 1]])``.
    ``X`` (numpy array or tensor, (N, D), D <= 256); a tensor on the device gives the same bits as the numpy array.  ``stats`` (a dict, optional) receives
    the k-NN phase's counters and ``steps``, the launches of the walk."""
    n, width = knn._shape_of(X)
    if width > MAX_DIM:
        raise NotImplementedError('hdbscan: at most %d features (got %d)' % (MAX_DIM, width))
    if isinstance(min_samples, bool) or not isinstance(min_samples, numbers.Integral) or min_samples < 1:
        raise ValueError('min_samples must be an int >= 1, got %r' % (min_samples,))
    k = int(min_samples)
    if k > n:
        raise ValueError('min_samples (%d) must be at most the number of samples in X (%d)' % (k, n))
    x = _device_points(X)
    core = knn.kth_neighbor_distance(x, k, stats=stats)
    ordering, reach, pred = device_walk(x, core, 'dic_hdbscan_workspace', 'dic_hdbscan_mst', stats=stats)
    return ordering, core, reach, pred


def single_linkage_tree(ordering, reach):
    """sklearn's ``_process_mst`` with a stable sort: the edges ``(ordering[i], ordering[i + 1], reach[ordering[i + 1]])`` of Prim's walk, sorted by weight
    (equal weights keep the walk's order), merged by union-find (``make_single_linkage``).  (N - 1,) ``HIERARCHY_dtype``: row i joins the clusters
    ``left_node`` and ``right_node`` (points < N, earlier rows j as N + j) at ``value`` into cluster N + i of ``cluster_size`` points."""
    ordering, reach = np.asarray(ordering, dtype=np.int64), np.asarray(reach, dtype=np.float64)
    n = len(ordering)
    weight = reach[ordering[1:]]
    order = np.argsort(weight, kind='stable')
    cur, nxt, weight = ordering[:-1][order].tolist(), ordering[1:][order].tolist(), weight[order]
    parent = [-1] * (2 * n - 1)
    size = [1] * n + [0] * (n - 1)
    left, right, count = [0] * (n - 1), [0] * (n - 1), [0] * (n - 1)
    for i in range(n - 1):
        pair = []
        for node in (cur[i], nxt[i]):
            top = node
            while parent[top] != -1:
                top = parent[top]
            while parent[node] != top and node != top:          # the shortcut up to the top
                parent[node], node = top, parent[node]
            pair.append(top)
        a, b = pair
        label = n + i
        parent[a] = parent[b] = label
        size[label] = size[a] + size[b]
        left[i], right[i], count[i] = a, b, size[label]
    out = np.zeros(n - 1, dtype=HIERARCHY_dtype)
    out['left_node'], out['right_node'], out['value'], out['cluster_size'] = left, right, weight, count
    return out


def _bfs_from_hierarchy(left, right, n, root):
    """The nodes below ``root`` (it included), level by level -- ``_tree.pyx: bfs_from_hierarchy``."""
    level, out = [root], []
    while level:
        out.extend(level)
        nxt = []
        for x in level:
            if x >= n:
                nxt.append(left[x - n])
                nxt.append(right[x - n])
        level = nxt
    return out


def condense_tree(hierarchy, min_cluster_size=10):
    """``_tree.pyx: _condense_tree``: the single-linkage tree with every split that sheds fewer than ``min_cluster_size`` points turned into those points
    leaving their cluster.  ``CONDENSED_dtype`` rows (parent, child, lambda = 1 / distance, size): children < N are points, the others clusters (the root
    is N)."""
    left, right = hierarchy['left_node'].tolist(), hierarchy['right_node'].tolist()
    value, count = hierarchy['value'].tolist(), hierarchy['cluster_size'].tolist()
    n = len(left) + 1
    root = 2 * (n - 1)
    next_label = n + 1
    relabel = [0] * (root + 1)
    relabel[root] = n
    ignore = [False] * (root + 1)
    rows = []
    for node in _bfs_from_hierarchy(left, right, n, root):
        if ignore[node] or node < n:
            continue
        lo, hi, distance = left[node - n], right[node - n], value[node - n]
        lam = 1.0 / distance if distance > 0.0 else np.inf
        lo_count = count[lo - n] if lo >= n else 1
        hi_count = count[hi - n] if hi >= n else 1
        here = relabel[node]
        if lo_count >= min_cluster_size and hi_count >= min_cluster_size:
            relabel[lo] = next_label
            next_label += 1
            rows.append((here, relabel[lo], lam, lo_count))
            relabel[hi] = next_label
            next_label += 1
            rows.append((here, relabel[hi], lam, hi_count))
            continue
        shed = []
        if lo_count < min_cluster_size:
            shed.append(lo)
        else:
            relabel[lo] = here
        if hi_count < min_cluster_size:
            shed.append(hi)
        else:
            relabel[hi] = here
        for top in shed:
            for sub in _bfs_from_hierarchy(left, right, n, top):
                if sub < n:
                    rows.append((here, sub, lam, 1))
                ignore[sub] = True
    return np.array(rows, dtype=CONDENSED_dtype)


def _compute_stability(parent, child, lam, size):
    smallest = min(parent)
    births = [np.nan] * (max(max(child), smallest) + 1)
    for c, v in zip(child, lam):
        births[c] = v
    births[smallest] = 0.0
    result = [0.0] * (max(parent) - smallest + 1)
    with np.errstate(invalid='ignore'):
        for p, v, s in zip(parent, lam, size):
            result[p - smallest] += (np.float64(v) - births[p]) * s
    return {i + smallest: float(v) for i, v in enumerate(result)}


def _max_lambdas(parent, lam):
    """``_tree.pyx: max_lambdas``: per cluster the largest lambda at which something left it (the rows of a parent are consecutive)."""
    deaths = [0.0] * (max(parent) + 1)
    current, top = parent[0], lam[0]
    for p, v in zip(parent[1:], lam[1:]):
        if p == current:
            top = max(top, v)
        else:
            deaths[current] = top
            current, top = p, v
    deaths[current] = top
    return deaths


class _TreeUnionFind:
    """``_tree.pyx: TreeUnionFind`` (union by rank)."""

    def __init__(self, size):
        self.up = list(range(size))
        self.rank = [0] * size

    def find(self, x):
        top = x
        while self.up[top] != top:
            top = self.up[top]
        while self.up[x] != top:
            self.up[x], x = top, self.up[x]
        return top

    def union(self, x, y):
        x, y = self.find(x), self.find(y)
        if self.rank[x] < self.rank[y]:
            self.up[x] = y
        elif self.rank[x] > self.rank[y]:
            self.up[y] = x
        else:
            self.up[y] = x
            self.rank[x] += 1


class _ClusterTree:
    """The rows of the condensed tree whose child is a cluster, with the look-ups ``_get_clusters`` makes on them."""

    def __init__(self, parent, child, lam, size):
        rows = [i for i, s in enumerate(size) if s > 1]
        self.parent, self.child = [parent[i] for i in rows], [child[i] for i in rows]
        self.lam, self.size = [lam[i] for i in rows], [size[i] for i in rows]
        self.children = {}
        for p, c in zip(self.parent, self.child):
            self.children.setdefault(p, []).append(c)
        self.row_of = {c: i for i, c in enumerate(self.child)}

    def __len__(self):
        return len(self.child)

    def below(self, root):
        """``bfs_from_cluster_tree``: root and every cluster under it."""
        out, level = [], [root]
        while level:
            out.extend(level)
            level = [c for p in level for c in self.children.get(p, ())]
        return out

    def leaves(self):
        if not len(self):
            return []
        out, stack = [], [min(self.parent)]
        while stack:
            node = stack.pop()
            kids = self.children.get(node)
            if kids:
                stack.extend(reversed(kids))
            else:
                out.append(node)
        return out

    def traverse_upwards(self, epsilon, leaf, allow_single_cluster):
        root = min(self.parent)
        while True:
            parent = self.parent[self.row_of[leaf]]
            if parent == root:
                return parent if allow_single_cluster else leaf          # the node closest to the root
            parent_eps = 1 / np.float64(self.lam[self.row_of[parent]])
            if parent_eps > epsilon:
                return parent
            leaf = parent

    def epsilon_search(self, leaves, epsilon, allow_single_cluster):
        selected, processed = [], set()
        for leaf in leaves:
            eps = 1 / np.float64(self.lam[self.row_of[leaf]])
            if eps < epsilon:
                if leaf not in processed:
                    top = self.traverse_upwards(epsilon, leaf, allow_single_cluster)
                    selected.append(top)
                    processed.update(sub for sub in self.below(top) if sub != top)
            else:
                selected.append(leaf)
        return set(selected)


def _do_labelling(parent, child, lam, clusters, cluster_map, allow_single_cluster, epsilon):
    root = min(parent)
    uf = _TreeUnionFind(max(parent) + 1)
    for p, c in zip(parent, child):
        if c not in clusters:
            uf.union(p, c)
    single = len(clusters) == 1 and allow_single_cluster
    if single:
        own = dict(zip(child, lam))          # (a child has one row)
        threshold = 1 / np.float64(epsilon) if epsilon != 0.0 else max(v for p, v in zip(parent, lam) if p == root)
    labels = np.empty(root, dtype=np.intp)
    for point in range(root):
        cluster = uf.find(point)
        label = NOISE
        if cluster != root:
            label = cluster_map[cluster]
        elif single and own[point] >= threshold:
            label = cluster_map[cluster]
        labels[point] = label
    return labels


def _get_probabilities(parent, child, lam, reverse_map, labels):
    out = np.zeros(len(labels))
    deaths = _max_lambdas(parent, lam)
    root = min(parent)
    for c, v in zip(child, lam):
        if c >= root:
            continue
        number = labels[c]
        if number == -1:
            continue
        top = deaths[reverse_map[number]]
        if top == 0.0 or np.isinf(v):
            out[c] = 1.0
        else:
            out[c] = min(v, top) / top
    return out


def _get_clusters(condensed, stability, method, allow_single_cluster, epsilon, max_cluster_size):
    """``_tree.pyx: _get_clusters``: ``(labels, probabilities)`` of the flat clustering the selection method takes from the condensed tree."""
    parent, child = condensed['parent'].tolist(), condensed['child'].tolist()
    lam, size = condensed['value'].tolist(), condensed['cluster_size'].tolist()
    node_list = sorted(stability, reverse=True)          # numeric id order is a topological order of the tree
    if not allow_single_cluster:
        node_list = node_list[:-1]          # (the root)
    tree = _ClusterTree(parent, child, lam, size)
    is_cluster = {c: True for c in node_list}
    n = max(c for c, s in zip(child, size) if s == 1) + 1
    if max_cluster_size is None:
        max_cluster_size = n + 1          # never reached
    sizes = dict(zip(tree.child, tree.size))
    if allow_single_cluster:
        sizes[node_list[-1]] = sum(s for p, s in zip(tree.parent, tree.size) if p == node_list[-1])
    if method == 'eom':
        for node in node_list:
            below = np.sum([stability[c] for c in tree.children.get(node, ())])
            if below > stability[node] or sizes[node] > max_cluster_size:
                is_cluster[node] = False
                stability[node] = below
            else:
                for sub in tree.below(node):
                    if sub != node:
                        is_cluster[sub] = False
        if epsilon != 0.0 and len(tree) > 0:
            eom = [c for c in is_cluster if is_cluster[c]]
            selected = []
            if len(eom) == 1 and eom[0] == min(tree.parent):          # the root alone: no epsilon check
                if allow_single_cluster:
                    selected = eom
            else:
                selected = tree.epsilon_search(set(eom), epsilon, allow_single_cluster)
            for c in is_cluster:
                is_cluster[c] = c in selected
    elif method == 'leaf':
        leaves = set(tree.leaves())
        if not leaves:
            for c in is_cluster:
                is_cluster[c] = False
            is_cluster[min(parent)] = True
        selected = tree.epsilon_search(leaves, epsilon, allow_single_cluster) if epsilon != 0.0 else leaves
        for c in is_cluster:
            is_cluster[c] = c in selected
    else:
        raise ValueError("cluster_selection_method must be 'eom' or 'leaf', got %r" % (method,))
    clusters = {c for c in is_cluster if is_cluster[c]}
    cluster_map = {c: i for i, c in enumerate(sorted(clusters))}
    reverse_map = {i: c for c, i in cluster_map.items()}
    labels = _do_labelling(parent, child, lam, clusters, cluster_map, allow_single_cluster, epsilon)
    return labels, _get_probabilities(parent, child, lam, reverse_map, labels)


def tree_to_labels(single_linkage, min_cluster_size=10, cluster_selection_method='eom', allow_single_cluster=False, cluster_selection_epsilon=0.0,
                   max_cluster_size=None, condensed=None):
    """``_tree.pyx: tree_to_labels``: ``(labels (N,) intp, probabilities (N,) f64)`` -- condense, compute the stabilities, select ('eom': the clusters of
    largest total stability; 'leaf': the leaves of the condensed tree; either merged upwards below ``cluster_selection_epsilon``), label.  ``condensed``: the
    ``condense_tree`` of the same arguments, where the caller has it already."""
    if condensed is None:
        condensed = condense_tree(single_linkage, min_cluster_size)
    stability = _compute_stability(condensed['parent'].tolist(), condensed['child'].tolist(), condensed['value'].tolist(), condensed['cluster_size'].tolist())
    return _get_clusters(condensed, stability, cluster_selection_method, bool(allow_single_cluster), float(cluster_selection_epsilon), max_cluster_size)


def labelling_at_cut(linkage, cut, min_cluster_size):
    """``_tree.pyx: labelling_at_cut``: the DBSCAN* labels at ``cut`` -- the components of the tree's edges lighter than ``cut``, those of fewer than
    ``min_cluster_size`` points noise, the others numbered in the order of their union-find roots."""
    left, right, value = linkage['left_node'].tolist(), linkage['right_node'].tolist(), linkage['value'].tolist()
    n = len(left) + 1
    uf = _TreeUnionFind(2 * (n - 1) + 1)
    for i in range(n - 1):
        if value[i] < cut:
            uf.union(left[i], n + i)
            uf.union(right[i], n + i)
    found = np.array([uf.find(p) for p in range(n)], dtype=np.intp)
    roots, inverse, counts = np.unique(found, return_inverse=True, return_counts=True)
    kept = counts >= min_cluster_size
    number = np.where(kept, np.cumsum(kept) - 1, NOISE).astype(np.intp)
    return number[inverse.reshape(-1)]


def _check_interval(name, value, kind, low, closed_low=True, none_ok=False, none_first=False):
    """sklearn's ``Interval`` constraint with its message."""
    real = kind is numbers.Real
    ok = not isinstance(value, bool) and isinstance(value, kind) and (value >= low if closed_low else value > low)
    if real and isinstance(value, numbers.Real) and not isinstance(value, bool) and np.isnan(value):
        ok = False
    if ok or (none_ok and value is None):
        return
    span = '%s in the range %s%s, inf)' % ('a float' if real else 'an int', '[' if closed_low else '(', float(low) if real else low)
    if none_ok:
        span = 'None or ' + span if none_first else span + ' or None'
    raise ValueError("The %r parameter of HDBSCAN must be %s. Got %r instead." % (name, span, value))


class HDBSCAN:
    """``sklearn.cluster.HDBSCAN`` (euclidean, ``alpha`` = 1) on the MI355X: ``fit`` sets ``labels_``, ``probabilities_``, ``core_distances_``,
    ``ordering_``, ``reachability_``, ``predecessor_`` (Prim's walk, ``hdbscan_mst``), ``single_linkage_tree_`` and ``condensed_tree_`` -- what sklearn's fit
    on the f64 distance matrix with ``metric='precomputed'`` gives where its unstable sort of equal weights does not matter (module docstring)."""

    def __init__(self, min_cluster_size=5, min_samples=None, cluster_selection_epsilon=0.0, max_cluster_size=None, metric='euclidean', metric_params=None,
                 alpha=1.0, algorithm='auto', leaf_size=40, n_jobs=None, cluster_selection_method='eom', allow_single_cluster=False, store_centers=None,
                 copy=False):
        if metric == 'precomputed':
            raise NotImplementedError("metric='precomputed' is not supported: pass the points themselves -- the distances are recomputed on the GPU, "
                                      'which is what spares the N x N matrix')
        if metric not in ('euclidean', 'l2') or metric_params:
            raise NotImplementedError('only the euclidean metric is on the accelerated path')
        if alpha != 1:
            raise NotImplementedError('alpha != 1 is not on the accelerated path')
        if store_centers is not None:
            raise NotImplementedError('store_centers is not on the accelerated path')
        self.min_cluster_size, self.min_samples, self.cluster_selection_epsilon, self.max_cluster_size = (
            min_cluster_size, min_samples, cluster_selection_epsilon, max_cluster_size)
        self.metric, self.metric_params, self.alpha, self.algorithm, self.leaf_size, self.n_jobs = metric, metric_params, alpha, algorithm, leaf_size, n_jobs
        self.cluster_selection_method, self.allow_single_cluster, self.store_centers, self.copy = (
            cluster_selection_method, allow_single_cluster, store_centers, copy)
        self.stats_ = None

    def _validate(self):
        _check_interval('min_cluster_size', self.min_cluster_size, numbers.Integral, 2)
        _check_interval('min_samples', self.min_samples, numbers.Integral, 1, none_ok=True)
        _check_interval('cluster_selection_epsilon', self.cluster_selection_epsilon, numbers.Real, 0)
        _check_interval('max_cluster_size', self.max_cluster_size, numbers.Integral, 1, none_ok=True, none_first=True)
        if not isinstance(self.cluster_selection_method, str) or self.cluster_selection_method not in ('eom', 'leaf'):
            raise ValueError("The 'cluster_selection_method' parameter of HDBSCAN must be a str among {'eom', 'leaf'}. Got %r instead."
                             % (self.cluster_selection_method,))
        if not isinstance(self.allow_single_cluster, (bool, np.bool_)):
            raise ValueError("The 'allow_single_cluster' parameter of HDBSCAN must be an instance of 'bool' or an instance of 'numpy.%s'. Got %r instead."
                             % (np.bool_.__qualname__, self.allow_single_cluster))

    def _extract(self, min_cluster_size):
        condensed = condense_tree(self.single_linkage_tree_, min_cluster_size)
        labels, probabilities = tree_to_labels(self.single_linkage_tree_, min_cluster_size, self.cluster_selection_method, self.allow_single_cluster,
                                               self.cluster_selection_epsilon, self.max_cluster_size, condensed=condensed)
        return condensed, labels, probabilities

    def fit(self, X, y=None):
        self._validate()
        n, _ = knn._shape_of(X)
        if n == 1:
            raise ValueError('n_samples=1 while HDBSCAN requires more than one sample')
        k = self.min_cluster_size if self.min_samples is None else self.min_samples
        if k > n:
            raise ValueError('min_samples (%d) must be at most the number of samples in X (%d)' % (k, n))
        self.stats_ = {}
        self.ordering_, self.core_distances_, self.reachability_, self.predecessor_ = hdbscan_mst(X, int(k), self.stats_)
        self.single_linkage_tree_ = single_linkage_tree(self.ordering_, self.reachability_)
        self.condensed_tree_, self.labels_, self.probabilities_ = self._extract(self.min_cluster_size)
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def dbscan_clustering(self, cut_distance, min_cluster_size=5):
        """``sklearn.cluster.HDBSCAN.dbscan_clustering``: the DBSCAN* labels (no border points) at ``eps = cut_distance`` read off the fitted tree."""
        return labelling_at_cut(self.single_linkage_tree_, cut_distance, min_cluster_size)


def hdbscan_sizes(X, min_samples, min_cluster_sizes, **selection):
    """One tree, one extraction per ``min_cluster_size``: the tree does not depend on it, so a sweep costs host time only.  ``selection``: the other
    ``HDBSCAN`` parameters.  Returns the fitted ``HDBSCAN`` of the first size (its ``ordering_`` .. ``single_linkage_tree_`` serve all of them) and
    ``{size: (labels, probabilities)}``."""
    sizes = [min_cluster_sizes] if isinstance(min_cluster_sizes, numbers.Integral) else list(min_cluster_sizes)
    if not sizes:
        raise ValueError('min_cluster_sizes is empty')
    for m in sizes:
        _check_interval('min_cluster_size', m, numbers.Integral, 2)
    fit = HDBSCAN(min_cluster_size=int(sizes[0]), min_samples=min_samples, **selection).fit(X)
    out = {int(sizes[0]): (fit.labels_, fit.probabilities_)}
    for m in sizes[1:]:
        if int(m) not in out:
            out[int(m)] = fit._extract(int(m))[1:]
    return fit, out
