"""What p2_clustering_optK.py and p4_clustering_final.py share: the --cluster_method names, the validity indices of one labelling, the noise / silhouette
summary of a density clustering and two small argument / tensor helpers.  Plain functions; the branch classes stay in the two programs, where the tests
patch the names they call."""
import numpy as np
import torch

from . import cluster_stats
from .internal_eval import CHIndex, DBIndex, DunnIndex, Sihouette
from .utils import logger

# every --cluster_method either program accepts: p2 has no 'dl' branch, p4 no 'optics' branch (both raise once the data are loaded)
METHODS = ('kmeans', 'dbscan', 'dl', 'optics', 'consensus', 'hdbscan', 'ward', 'gmm', 'fcm', 'snn', 'spectral', 'meanshift', 'kmedoids', 'densitypeaks', 'bgmm')

INDICES = {'Dunn_Index': DunnIndex, 'Sihouette': Sihouette, 'Davies-Bouldin_Index': DBIndex, 'Calinski-Harabasz': CHIndex}


def spell(names):
    """'a, b and c' for an error message."""
    names = list(names)
    return ', '.join(names[:-1]) + ' and ' + names[-1]


def contamination_arg(text):
    """--outlier_contamination: 'auto' or a float (lof.py refuses one outside (0, 0.5])."""
    return text if text == 'auto' else float(text)


def device_latents(data):
    """The latents of a cohort dict as f32 on the current device."""
    return torch.as_tensor(data['hidden'], dtype=torch.float32, device=torch.device('cuda', torch.cuda.current_device()))


def build_metrics(names):
    """The validity-index callables of --internal_metrics, in the given order."""
    return [INDICES[n]() for n in names]


def metric_values(Xd, labels, metrics, metric_sample=0, stats=None, nan_below_two=False):
    """The values of ``metrics`` (``build_metrics``) for the 0-based ``labels`` of the device points ``Xd``, in their order.  ``metric_sample`` below
    len(labels): the indices of that many points drawn by RandomState(0), each index with its own pair pass.  Else ONE pair pass shared by all of them
    (``stats``: the caller's, where it has one already), with the min / max terms only where the Dunn index asks for them.  Fewer than two clusters raise
    ValueError (cluster_stats) unless ``nan_below_two``: then every value is NaN -- for the branches whose fit can come back with one cluster."""
    if nan_below_two and (labels.size == 0 or labels.max() < 1):          # (the indices need two clusters)
        return [float('nan')] * len(metrics)
    if metric_sample and metric_sample < len(labels):
        pick = np.random.RandomState(0).choice(len(labels), metric_sample, replace=False)
        Xs = Xd[torch.as_tensor(pick, device=Xd.device)]
        return [m(Xs, labels[pick]) for m in metrics]
    if stats is None:
        need_minmax = any(isinstance(m, DunnIndex) for m in metrics)
        stats = cluster_stats.pair_stats(Xd, labels, need_min=need_minmax, need_max=need_minmax)
    return [m(Xd, labels, stats=stats) for m in metrics]


def metric_log(names, vals):
    """'name: value' of every index, the tail of a per-K log line."""
    return ' '.join('{}: {:.4f}'.format(n, v) for n, v in zip(names, vals))


DBCV_COLUMNS = ['labelling', 'n_clusters', 'n_noise', 'n_singletons', 'dbcv']
DBCV_CLUSTER_COLUMNS = ['labelling', 'cluster', 'size', 'sparseness', 'separation', 'nearest_cluster', 'validity']


def dbcv_summary(points, labellings):
    """--validity dbcv: the DBCV (dbcv.py) of every entry of ``labellings`` ({name: (N,) int labels, -1 for noise}) on ``points`` (a device tensor or a
    NumPy array, uploaded once), logged, as two lists of rows: ``DBCV_COLUMNS`` -- one per labelling, NaN where it has fewer than two clusters of two
    members -- and ``DBCV_CLUSTER_COLUMNS``, one per kept cluster.  The exponent is the column count of ``points``."""
    from . import dbcv          # (here, not at module scope: a run without --validity loads nothing of it)
    x, width = dbcv._points(points)
    rows, cluster_rows = [], []
    for name, labels in labellings.items():
        labels = np.asarray(labels).astype(np.int64)
        try:
            res = dbcv._score(x, width, labels, None)
        except ValueError as e:
            logger.info('DBCV of {}: not defined ({})'.format(name, e))
            ids, counts = np.unique(labels[labels != -1], return_counts=True)
            rows.append((name, int((counts >= 2).sum()), int((labels == -1).sum()), int((counts == 1).sum()), float('nan')))
            continue
        rows.append((name, len(res.cluster_ids), res.n_noise, res.n_singletons, res.score))
        cluster_rows += [(name, int(c), int(n), s, p, int(q), v) for c, n, s, p, q, v in
                         zip(res.cluster_ids, res.sizes, res.sparseness, res.separation, res.nearest_cluster, res.validity)]
        logger.info('DBCV of {}: {:.6f}, clusters: {}, noise: {}, singletons: {}'.format(name, res.score, len(res.cluster_ids), res.n_noise, res.n_singletons))
    return rows, cluster_rows


AGREEMENT_INDICES = ('ari', 'ami', 'nmi', 'rand', 'fmi', 'vmeasure')
AGREEMENT_COLUMNS = ['labelling_a', 'labelling_b', 'n', 'clusters_a', 'clusters_b']          # (then the requested indices, in the order asked for)


def add_agreement_arguments(p, what):
    """The three --agreement flags of p2 and p4; ``what``: which labellings the program compares, for the help text."""
    p.add_argument('--agreement', nargs='+', default=None, choices=list(AGREEMENT_INDICES), metavar='INDEX',
                   help='(extra) also compare {} with each other by these indices ({})'.format(what, ' '.join(AGREEMENT_INDICES)))
    p.add_argument('--agreement_scope', default='all', choices=['all', 'method'],
                   help="(extra) --agreement: the labellings of every method's output directory that exists (all, the default) or of this --cluster_method only")
    p.add_argument('--agreement_noise', default='class', choices=['class', 'drop'],
                   help="(extra) --agreement: -1 is a class like any other (class, sklearn's behaviour) or, per pair, rows with -1 in either labelling are left out")


def agreement_summary(labellings, indices, noise='class'):
    """--agreement: every unordered pair of ``labellings`` ({name: (N,) int labels}; uploaded once) compared by ``indices`` (agreement.py), one log line
    per pair.  Returns the rows of the long table -- ``AGREEMENT_COLUMNS`` then the indices -- and ``{index: (L, L) matrix}``, the diagonal from the same
    kernels."""
    from . import agreement          # (here, not at module scope: a run without --agreement loads nothing of it)
    indices = list(indices)
    res = agreement.agreement_matrix(labellings, indices=indices, noise=noise)
    rows = []
    for p, (i, j) in enumerate(res.pairs):
        vals = [float(res.values[name][p]) for name in indices]
        rows.append((res.names[i], res.names[j], int(res.n[p]), int(res.n_clusters[p, 0]), int(res.n_clusters[p, 1])) + tuple(vals))
        logger.info('agreement of {} and {}: rows: {}, clusters: {} / {}, {}'.format(res.names[i], res.names[j], int(res.n[p]), int(res.n_clusters[p, 0]),
                                                                                      int(res.n_clusters[p, 1]), metric_log(indices, vals)))
    return rows, {name: res[name] for name in indices}


def _integer_columns(csv, prefix, n_rows, out):
    """Adds the columns of a label table to ``out`` as ``<prefix>:<column>``; a file of another row count, or a column that holds no integers, is logged
    and skipped."""
    import pandas as pd
    table = pd.read_csv(csv)
    if len(table) != n_rows:
        logger.info('No agreement for {}: {} rows against the {} of the training cohort.'.format(csv, len(table), n_rows))
        return
    for column in table.columns:
        values = table[column].to_numpy()
        if not np.issubdtype(values.dtype, np.integer):
            logger.info('No agreement for column {} of {}: it holds no integers.'.format(column, csv))
            continue
        out['{}:{}'.format(prefix, column)] = values.astype(np.int64)


def training_labellings(out_feat, metric, methods, n_rows, consensus=True):
    """p2 --agreement: ``{'<method>:<column>': labels}`` from every ``<out_feat>/<metric>_<m>_aligned/plot/<m>_labels.csv`` that exists for m in ``methods``,
    and with ``consensus`` the columns of ``<out_feat>/raw_consensus_result/training_consensus.csv`` as ``consensus:k<K>``."""
    import os.path as osp
    out = {}
    for m in methods:
        csv = osp.join(out_feat, '{}_{}_aligned'.format(metric, m), 'plot', '{}_labels.csv'.format(m))
        if osp.exists(csv):
            _integer_columns(csv, m, n_rows, out)
    raw = osp.join(out_feat, 'raw_consensus_result', 'training_consensus.csv')
    if consensus and osp.exists(raw):
        _integer_columns(raw, 'consensus', n_rows, out)
    return out


def cohort_labellings(out_feat, metric, methods, cohort, encounter_id):
    """p4 --agreement: ``{'<method>/<file stem>': cluster_id}`` from every ``<out_feat>/<metric>_<m>_aligned/<cohort>_*.npy`` for m in ``methods`` that
    holds a ``cluster_id`` and the same ``encounter_id`` array as the cohort; any other file is logged and skipped."""
    import glob
    import os.path as osp
    out = {}
    encounter_id = np.asarray(encounter_id)
    for m in methods:
        for f in sorted(glob.glob(osp.join(out_feat, '{}_{}_aligned'.format(metric, m), '{}_*.npy'.format(cohort)))):
            try:
                saved = np.load(f, allow_pickle=True).item()
            except (ValueError, AttributeError):          # (an array, not a dict: a map)
                saved = None
            if not isinstance(saved, dict) or 'cluster_id' not in saved or 'encounter_id' not in saved:
                continue
            ids = np.asarray(saved['cluster_id'])
            if not np.array_equal(np.asarray(saved['encounter_id']), encounter_id) or ids.shape != encounter_id.shape or not np.issubdtype(ids.dtype, np.integer):
                logger.info('No agreement for {}: other encounters than the {} cohort, or no integer labels.'.format(f, cohort))
                continue
            out['{}/{}'.format(m, osp.splitext(osp.basename(f))[0])] = ids.astype(np.int64)
    return out


def noise_summary(points, labels, n_core=None):
    """Logs what upstream's Dbscan.train logs of one labelling with noise (-1) -- the core count where one is given, the clusters, the noise points, then
    either that the silhouette is skipped (one cluster) or the silhouette of all points and of the points without noise -- and returns ``(n_clusters,
    n_noise, silhouette, denoise_silhouette)``, the last two NaN where they were not computed (fewer than two clusters).  ``points``: a device tensor or
    a NumPy array, handed to ``cluster_stats.silhouette_score`` as it is."""
    if n_core is not None:
        logger.info('core_sample: {}'.format(n_core))
    n_clusters = len(set(labels.tolist())) - (1 if -1 in labels else 0)
    n_noise = int(np.sum(labels == -1))
    logger.info('Estimated number of clusters: %d' % n_clusters)
    logger.info('Estimated number of noise points: %d' % n_noise)
    sil = sil_dn = float('nan')
    if n_clusters == 1:
        logger.info('Skip the Silhouette Coefficient calculation.')
    elif n_clusters > 1:
        keep = labels != -1
        sil = cluster_stats.silhouette_score(points, labels)
        sil_dn = cluster_stats.silhouette_score(points[torch.as_tensor(keep, device=points.device)] if torch.is_tensor(points) else points[keep], labels[keep])
        logger.info('Orginal Sample: {} Silhouette Coefficient: {:.5f}'.format(len(labels), sil))
        logger.info('Denoise sample: {}, Denoise Silhouette Coefficient: {:.5f}'.format(int(keep.sum()), sil_dn))
    return n_clusters, n_noise, sil, sil_dn
