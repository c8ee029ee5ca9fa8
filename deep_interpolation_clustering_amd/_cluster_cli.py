"""What p2_clustering_optK.py and p4_clustering_final.py share: the --cluster_method names, the validity indices of one labelling, the noise / silhouette
summary of a density clustering and two small argument / tensor helpers.  Plain functions; the branch classes stay in the two programs, where the tests
patch the names they call."""
import numpy as np
import torch

from . import cluster_stats
from .internal_eval import CHIndex, DBIndex, DunnIndex, Sihouette
from .utils import logger

# every --cluster_method either program accepts: p2 has no 'dl' branch, p4 no 'optics' branch (both raise once the data are loaded)
METHODS = ('kmeans', 'dbscan', 'dl', 'optics', 'consensus', 'hdbscan', 'ward', 'gmm', 'snn', 'spectral', 'meanshift', 'kmedoids', 'densitypeaks')

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
