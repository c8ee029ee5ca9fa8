"""p2: choose the number of clusters on the saved latents -- elbow and gap statistic over k = 2..k_max
(p2_clustering_optK.py:225-410) with every k-means fit on the HIP kernels.

    cd <run dir>;  python -m deep_interpolation_clustering_amd.p2_clustering_optK --k_max 10

Reads Results/Pretrain/out_feat/<metric>/<cohort>.npy (written by p1), writes
Results/Pretrain/out_feat/<metric>_kmeans_aligned/plot/{elbow.csv, gap_sts_v1.csv}.  The gap statistic's
"mean intra-cluster pairwise distance" and the validity indices come from one tiled all-pairs pass on the GPU
(cluster_stats.py / csrc/dic_pairdist.hip) instead of an n_c x n_c float64 matrix per cluster (multi-GB at 75 k points).

``--cluster_method dbscan`` (p2:82-85,90-168): DBSCAN for eps = 0.5, 1.0, .., 5.0 and min_samples = feat_dim + 1 on the GPU (dbscan.py: no N x N
distance matrix), with the core / cluster / noise counts and both silhouettes per eps, written to <metric>_dbscan_aligned/plot/dbscan_eps.csv.  With
--select_eps k_distance_graph (the default; p2:102-120) the feat_dim-NN distance curve of the training latents and its elbow -- the eps p4's --opt_eps is
meant to be -- go to plot/k_distance.csv and plot/k_distance_elbow.csv (knn.py).

``--cluster_method optics`` (p2:86-88,171-223): OPTICS with min_samples = feat_dim + 1 and the xi extraction (xi = .05, min_cluster_size = min_samples) on
the GPU (optics.py: no N x N matrix, one launch per step of the main loop).  In place of the reachability plot its data go to
<metric>_optics_aligned/plot/reachability_xi.csv (x, sample, dist, label: position in the ordering, point index, reachability, label -- every point, noise
included) and the summary to plot/optics_xi.csv (min_samples, n_clusters, n_noise).  ONE DELIBERATE DEPARTURE: upstream calls
``optics.fit(train_feat_dist)`` with the default metric (p2:196), which clusters the ROWS OF THE DISTANCE MATRIX as N-dimensional feature vectors; the
commented-out ``optics.fit(train_feat)`` above it (p2:195) is the intent, and here OPTICS runs on the latents themselves.

``--cluster_method consensus``: upstream has no such fit -- its p4 reads out_feat/raw_consensus_result/<cohort>_consensus.csv (columns k2, k3, ..), labels
"generated outside" (p4_clustering_final.py:241-287).  Here they are generated: consensus clustering with a k-means base clusterer for K = 2..k_max
(consensus.py: --consensus_reps resamples of --consensus_p_item of the points, the pair consensus, its CDF and the average-linkage cut on the GPU) on the
training latents, whose CDFs go to <metric>_consensus_aligned/plot/consensus_cdf.csv (k, c, cdf) and the areas under them to plot/consensus_area.csv (k,
area, delta_area); the 1-based labels of the training and of the validation cohort, each clustered on its own as the outside step did, go to
out_feat/raw_consensus_result/{training,validation}_consensus.csv in the format p4 reads.

``--cluster_method hdbscan`` (no upstream counterpart): HDBSCAN with min_samples = feat_dim + 1 on the training latents on the GPU (hdbscan.py: no N x N
matrix, one launch per step of Prim's walk over the mutual-reachability graph), extracted for every --hdbscan_min_cluster_size (default feat_dim + 1; the
tree does not depend on it).  The walk goes to <metric>_hdbscan_aligned/plot/hdbscan_mst.csv (x, sample, source, dist: position in the walk, point index,
its neighbour in the tree, the weight it joined at), the per-size table to plot/hdbscan_sizes.csv (min_cluster_size, n_clusters, n_noise, silhouette,
denoise_silhouette) and the labels to plot/hdbscan_labels.csv, one column mcs<size> per size.

``--cluster_method ward`` (no upstream counterpart): Ward's agglomerative clustering of the training latents on the GPU (ward.py: no N x N matrix, one launch
per step of the nearest-neighbour chain over the live centroids).  ONE tree serves every K: it is cut at K = 2..k_max, and per K the merge height, the mean
distance to the nearest centre on the training and the validation latents (the elbow's distortion) and the --internal_metrics go to
<metric>_ward_aligned/plot/ward_k.csv; the dendrogram goes to plot/ward_linkage.csv (scipy's Z, %.17g) and the 0-based labels to plot/ward_labels.csv, one
column k<K> per K.

``--cluster_method gmm`` (no upstream counterpart): Gaussian mixtures with --gmm_covariance_type diag | spherical | full | tied covariances, fitted to the training latents on
the GPU for K = 2..k_max with --n_init restarts each (gmm.py: f64 EM, one pass over the latents per iteration, the restarts advancing together).  Per K the
lower bound, BIC and AIC of the fit itself -- a likelihood-based criterion for K that needs no reference sets -- the iterations, the mean log-likelihood of the
validation cohort and the --internal_metrics of the hard labels go to <metric>_gmm_aligned/plot/gmm_k.csv, the 0-based labels to plot/gmm_labels.csv, one
column k<K> per K.

``--cluster_method fcm`` (no upstream counterpart): fuzzy c-means (fcm.py: Bezdek's soft partition, memberships from distance ratios alone, the post-hoc
counterpart of DEC's q) of the training latents on the GPU for K = 2..k_max with --n_init restarts each, one sweep per fuzzifier of --fcm_m (default 2; closer
to 1 is harder).  Per (m, K) the objective J, the partition coefficient, its modified form, the partition entropy, Xie-Beni and the fuzzy silhouette -- criteria
for K that need no likelihood --, the iterations, the number of coincident centre pairs (a collapsed fit: in high dimensions FCM runs all centres together,
and the remedy is a smaller m), the partition coefficient of the validation cohort under the training centres and the --internal_metrics of the hard labels go
to <metric>_fcm_aligned/plot/fcm_k.csv, the 0-based labels to plot/fcm_labels.csv, one column m<m>_k<K> per fit, and the centres to plot/fcm_centers.csv (m, k,
cluster, the coordinates), %.17g.

``--cluster_method bgmm`` (no upstream counterpart): variational Bayesian Gaussian mixtures (bgmm.py) of k_max components, one fit per value of
--bgmm_concentration (default 1 / k_max) with --n_init restarts, --gmm_covariance_type diag | spherical and --bgmm_prior_type dirichlet_process |
dirichlet_distribution: the prior empties the components the latents do not support, so ONE fit answers how many there are.  Per concentration the active
components, the lower bound, the iterations, the validation score and the --internal_metrics of the hard labels go to <metric>_bgmm_aligned/plot/bgmm_k.csv,
the per-component weights to plot/bgmm_weights.csv and the labels -- the active components renumbered 0..A-1 -- to plot/bgmm_labels.csv, one column per
concentration.

``--cluster_method snn`` (no upstream counterpart): shared-nearest-neighbour clustering of the training latents on the GPU (snn.py: the k-neighbour lists of
knn.py, one pass over them for the similarities, no N x N matrix) -- closeness counted in shared neighbours, an integer without a scale, where the euclidean
eps of the dbscan branch flips from all noise to one cluster within a narrow band.  ONE graph with k = --snn_k (default feat_dim + 1) serves every
--snn_eps (default round(k t / 10) for t = 2..8) at --snn_min_samples (default k // 4); the per-eps table -- the dbscan branch's columns plus k and
min_samples -- goes to <metric>_snn_aligned/plot/snn_eps.csv, the list entries per similarity 0..k -- the curve eps is read from, as the k-distance graph is
for DBSCAN -- to plot/snn_similarity_hist.csv (similarity, pairs) and the labels to plot/snn_labels.csv, one column eps<eps> per eps.  The defaults of
--snn_eps and --snn_min_samples are starting points: nobody has measured them on the real latents.
``--cluster_method spectral`` (no upstream counterpart): spectral clustering of the training latents on the GPU (spectral.py: the symmetrised --spectral_k
neighbour graph, default 10 as in sklearn, and the largest eigenpairs of its normalised adjacency by Chebyshev-filtered subspace iteration).  ONE graph and ONE
decomposition with k_max + 1 eigenpairs serve K = 2..k_max: the labels of K come from the first K eigenvectors by --spectral_assign kmeans | cluster_qr.  The
eigenvalues and their gaps go to <metric>_spectral_aligned/plot/spectral_eigenvalues.csv (index, eigenvalue, eigengap: the gap to the next one, so the gap after
k_max is there), the per-K table (k, eigengap, n_iter, converged, n_connected_components and the --internal_metrics on the latents) to plot/spectral_k.csv and
the 0-based labels to plot/spectral_labels.csv, one column k<K> per K.  The default --spectral_k is a starting point: DESIGN.md records what it gives.

``--cluster_method meanshift`` (no upstream counterpart): mean shift with the flat kernel on the training latents on the GPU (meanshift.py: every point a seed
unless --meanshift_bin_seeding, all seeds advancing together, no N x N structure) -- the one family here that both picks the number of clusters itself and
gives centres to carry to the other cohorts.  One fit per bandwidth: --meanshift_bandwidth, or estimate_bandwidth at every --meanshift_quantile (default 0.1
0.2 0.3).  The per-bandwidth table (quantile, bandwidth, n_clusters, n_orphans, largest, smallest, n_iter, valid_distortion: the validation cohort's mean
distance to its nearest centre, and the --internal_metrics) goes to <metric>_meanshift_aligned/plot/meanshift_bandwidth.csv, the labels to
plot/meanshift_labels.csv, one column bw<index> per bandwidth, and the centres to plot/meanshift_centers.csv (bandwidth, cluster, the coordinates), %.17g.

``--cluster_method kmedoids`` (no upstream counterpart): k-medoids (PAM: BUILD, then steepest-descent SWAP) of the training latents on the GPU for
K = 2..k_max (kmedoids.py: no N x N matrix; an approximate pass on the matrix cores selects swap candidates, an exact f64 stage decides) -- the one family
whose centres are encounters.  The per-K table (k, inertia = the sum of distances to the nearest medoid, n_iter, converged and the --internal_metrics) goes
to <metric>_kmedoids_aligned/plot/kmedoids_k.csv, the 0-based labels to plot/kmedoids_labels.csv, one column k<K> per K, and the medoids to
plot/kmedoids_medoids.csv (k, cluster, the row of the medoid encounter in the training latents, its encounter id).

``--cluster_method densitypeaks`` (no upstream counterpart): density-peaks clustering (Rodriguez and Laio 2014) of the training latents on the GPU
(density_peaks.py: no N x N matrix) -- the one family that shows a picture from which the number of phenotypes is read.  ONE computation of rho (--dp_density
cutoff | knn; d_c = --dp_dc or the --dp_percent rule), delta and parent; the decision graph goes to <metric>_densitypeaks_aligned/plot/
densitypeaks_decision.csv (index, rho, delta, gamma, parent for every point, %.17g), the per-K table for K = 2..--dp_k (default k_max) to
plot/densitypeaks_k.csv (k, gamma_gap = gamma_(K) / gamma_(K+1), sizes, n_halo and the --internal_metrics of the labels without the halo) and the 0-based
labels, -1 for halo points with --dp_halo 1, to plot/densitypeaks_labels.csv, one column k<K> per K.

``--embed tsne`` (no upstream counterpart; beside any --cluster_method): one exact t-SNE fit of the training latents on the GPU (tsne.py: --tsne_perplexity,
default 30, --tsne_max_iter, default 1000, init 'pca') -- the two-dimensional map every plot/*_labels.csv above can be drawn on.  The map goes to
<metric>_<method>_aligned/plot/tsne.csv (x, y as %.17g, one row per training encounter in the cohort's row order) and the error at every check to
plot/tsne_kl.csv (iteration, kl).  Without --embed nothing changes.  ``--embed_quality_k 5 10 30`` (with --embed tsne) also says whether the map's
neighbourhoods can be believed (embedding_quality.py): plot/tsne_quality.csv (k, trustworthiness, continuity, neighbors_kept as %.17g, one row per k), the
figures that are comparable across perplexities, which kl is not.  Without that flag no such file is written.

``--outlier lof`` (no upstream counterpart; beside any --cluster_method): the local outlier factor of every training encounter (lof.py: sklearn's
LocalOutlierFactor, exact for the f32 latents) at every k of --outlier_k (default 20) from ONE neighbour join.  plot/lof.csv has one row per training
encounter in the cohort's row order: per k ``lof_k<k>`` (the positive factor, -negative_outlier_factor_, as %.17g: about 1 inside a neighbourhood, larger
the more isolated) and ``outlier_k<k>`` (1 where the factor lies beyond the offset of --outlier_contamination: 'auto', the default, is 1.5; a float in
(0, 0.5] is that share of the cohort), and ``lof_max``, the largest factor over the given k (Breunig's range heuristic).  plot/lof_summary.csv has one
row per k: k, offset, n_outliers, max_lof.  Nothing is removed from any clustering branch: that stays a join on lof.csv.  Without --outlier nothing changes.

``--validity dbcv`` (no upstream counterpart; beside any --cluster_method): after the branch has run, every column of its plot/<method>_labels.csv is
scored against the training latents by DBCV (dbcv.py: Density-Based Clustering Validation, one number in [-1, 1] that has a place for noise and does not
reward convex blobs -- the figure by which labellings of different eps, min_cluster_size or methods can be compared).  plot/dbcv.csv has one row per
column: labelling, n_clusters, n_noise, n_singletons, dbcv (NaN below two clusters); plot/dbcv_clusters.csv one row per cluster: labelling, cluster, size,
sparseness, separation, nearest_cluster, validity; both %.17g.  A method that writes no such label file (kmeans, dbscan, optics, consensus) is logged and
skipped.  Without --validity nothing changes.

``--agreement INDEX [INDEX ...]`` (ari ami nmi rand fmi vmeasure; no upstream counterpart; beside any --cluster_method): after the branch and --validity
have run, the TRAINING labellings are compared with each other, every unordered pair (agreement.py: sklearn.metrics.cluster's indices, all pairs in one
launch per stage).  --agreement_scope method: the columns of this run's plot/<method>_labels.csv; all (the default): the columns of every
<metric>_<m>_aligned/plot/<m>_labels.csv that exists, and those of raw_consensus_result/training_consensus.csv as consensus:k<K>.  A labelling is named
<method>:<column>; a file of another row count than the training cohort is logged and skipped; fewer than two labellings: logged, nothing written.
--agreement_noise class (the default: -1 is a class, as in sklearn) or drop (per pair, rows with -1 in either labelling are left out).  plot/agreement.csv
has one row per pair: labelling_a, labelling_b, n, clusters_a, clusters_b, then the indices; plot/agreement_<index>.csv is the square table of one index,
the names as header and first column; all %.17g.  Without --agreement nothing changes.

The seaborn plots of the upstream script are not provided.
"""
import argparse
import os
import queue
import threading
import warnings
import os.path as osp

import numpy as np
import pandas as pd
import torch

from . import cluster_stats, dist
from ._cluster_cli import AGREEMENT_COLUMNS, DBCV_CLUSTER_COLUMNS, DBCV_COLUMNS, METHODS, add_agreement_arguments, agreement_summary, build_metrics, dbcv_summary, contamination_arg, device_latents, metric_log, metric_values, noise_summary, spell, training_labellings
from .consensus import BINS, ConsensusKMeans
from .dbscan import dbscan_sweep
from .density_peaks import density_peaks_sweep
from .fcm import fcm_sweep
from .bgmm import bgmm_sweep
from .gmm import gmm_sweep
from .gmm_full import gmm_full_sweep
from .hdbscan import hdbscan_sizes
from .info import COHORTS
from .internal_eval import DunnIndex
from .kmeans import KMeans, seed_draw_count
from .kmedoids import kmedoids_sweep
from .meanshift import estimate_bandwidth, mean_shift_sweep
from .knn import k_distance_graph
from .optics import OPTICS
from .snn import snn_sweep
from ._native import MAX_CLUSTERS
from .spectral import spectral_sweep
from .tsne import TSNE
from .utils import logger, print_dict_byline
from .ward import Ward as WardLinkage

np.random.seed(123)        # p2_clustering_optK.py:23


def get_arguments(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--cluster_method', default='kmeans', choices=METHODS)
    p.add_argument('--k_max', type=int, default=10, help='The max value of k, for k-means only.')
    p.add_argument('--select_opt_k', default=['gap_sts', 'elbow'])
    p.add_argument('--select_eps', type=str, default='k_distance_graph')
    p.add_argument('--n_init', type=int, default=10, help='The number of initialization for k-means.')
    p.add_argument('--gap_b', type=int, default=10, help='The number of randomly sampling for gap-sts.')
    p.add_argument('--restore_metric', default=['ae_mse', 'loss'])
    p.add_argument('--opt_eps', type=float, default=1.9)
    p.add_argument('--internal_metrics', default=['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz'])
    p.add_argument('--consensus_reps', type=int, default=100, help='(extra) resamples of the consensus clustering')
    p.add_argument('--consensus_p_item', type=float, default=0.8, help='(extra) fraction of the points in a resample')
    p.add_argument('--hdbscan_min_cluster_size', type=int, nargs='+', default=None,
                   help='(extra) min_cluster_size values of --cluster_method hdbscan; default feat_dim + 1')
    p.add_argument('--gmm_covariance_type', default='diag', choices=['diag', 'spherical', 'full', 'tied'],
                   help='(extra) covariances of --cluster_method gmm; full and tied run gmm_full.py (bgmm: diag or spherical)')
    p.add_argument('--fcm_m', type=float, nargs='+', default=[2.0],
                   help='(extra) fuzzifiers of --cluster_method fcm, each > 1, one sweep over K per value; default 2 -- where plot/fcm_k.csv reports '
                        'coincident centres (a collapsed fit, usual in high dimensions) choose a smaller one, e.g. 1.2')
    p.add_argument('--bgmm_concentration', type=float, nargs='+', default=None,
                   help='(extra) weight concentration priors of --cluster_method bgmm, one fit each (default: 1 / k_max)')
    p.add_argument('--bgmm_prior_type', default='dirichlet_process', choices=['dirichlet_process', 'dirichlet_distribution'],
                   help='(extra) the weight prior of --cluster_method bgmm')
    p.add_argument('--snn_k', type=int, default=None, help='(extra) neighbours per point of --cluster_method snn; default feat_dim + 1')
    p.add_argument('--snn_eps', type=int, nargs='+', default=None,
                   help='(extra) shared-neighbour thresholds of --cluster_method snn, integers in [1, k]; default round(k t / 10) for t = 2..8 -- a starting '
                        'point, not measured on the real latents: read eps from plot/snn_similarity_hist.csv')
    p.add_argument('--spectral_k', type=int, default=10, help="(extra) neighbours per point of --cluster_method spectral; default 10, sklearn's")
    p.add_argument('--spectral_assign', default='kmeans', choices=['kmeans', 'cluster_qr'], help='(extra) how --cluster_method spectral labels the embedding')
    p.add_argument('--snn_min_samples', type=int, default=None,
                   help='(extra) strong links that make a core point of --cluster_method snn (0: Jarvis-Patrick); default k // 4 -- a starting point, not '
                        'measured on the real latents')
    p.add_argument('--meanshift_quantile', type=float, nargs='+', default=[0.1, 0.2, 0.3],
                   help='(extra) quantiles of --cluster_method meanshift: one fit per bandwidth estimate_bandwidth(training latents, quantile)')
    p.add_argument('--meanshift_bandwidth', type=float, nargs='+', default=None, help='(extra) bandwidths of --cluster_method meanshift; overrides the quantiles')
    p.add_argument('--meanshift_bin_seeding', action='store_true', help="(extra) seed --cluster_method meanshift from sklearn's bins, not from every point")
    p.add_argument('--meanshift_cluster_all', type=int, default=1, choices=[1, 0],
                   help='(extra) 0: a point farther than the bandwidth from its nearest centre is an orphan (-1)')
    p.add_argument('--dp_density', default='cutoff', choices=['cutoff', 'knn'], help='(extra) density of --cluster_method densitypeaks')
    p.add_argument('--dp_percent', type=float, default=2.0,
                   help='(extra) --cluster_method densitypeaks: d_c is the radius at which a point has on average this percentage of the cohort as neighbours')
    p.add_argument('--dp_dc', type=float, default=None, help='(extra) d_c of --cluster_method densitypeaks; overrides --dp_percent')
    p.add_argument('--dp_k', type=int, default=None, help='(extra) the largest K of --cluster_method densitypeaks; default k_max')
    p.add_argument('--dp_halo', type=int, default=0, choices=[0, 1], help='(extra) 1: halo points of --cluster_method densitypeaks are labelled -1 (cutoff only)')
    p.add_argument('--metric_sample', type=int, default=0, help='(extra) subsample size for the O(N^2) validity indices; 0 = all')
    p.add_argument('--embed', default=None, choices=['tsne'],
                   help='(extra) also write a two-dimensional map of the training latents (plot/tsne.csv) that every plot/*_labels.csv can be drawn on')
    p.add_argument('--tsne_perplexity', type=float, default=30.0, help="(extra) perplexity of --embed tsne; default 30, sklearn's")
    p.add_argument('--tsne_max_iter', type=int, default=1000, help="(extra) iterations of --embed tsne; default 1000, sklearn's (250 of them exaggerated)")
    p.add_argument('--embed_quality_k', type=int, nargs='+', default=None,
                   help='(extra) with --embed tsne: also write trustworthiness, continuity and the share of neighbours kept of the map at these '
                        'neighbourhood sizes (plot/tsne_quality.csv), e.g. 5 10 30')
    p.add_argument('--outlier', default=None, choices=['lof'],
                   help='(extra) also write the local outlier factor of every training encounter (plot/lof.csv, plot/lof_summary.csv)')
    p.add_argument('--outlier_k', type=int, nargs='+', default=[20], help="(extra) neighbourhood sizes of --outlier lof, one join for all; default 20, sklearn's")
    p.add_argument('--validity', default=None, choices=['dbcv'],
                   help="(extra) also score every column of the method's plot/<method>_labels.csv by DBCV (plot/dbcv.csv, plot/dbcv_clusters.csv)")
    add_agreement_arguments(p, 'the training labellings on disk (plot/agreement.csv, plot/agreement_<index>.csv)')
    p.add_argument('--outlier_contamination', type=contamination_arg, default='auto',
                   help="(extra) --outlier lof: 'auto' (an encounter is an outlier beyond a factor of 1.5) or the share of outliers, a float in (0, 0.5]")
    return p.parse_args(argv)


def global_uniform_into(out):
    """``out[...] = np.random.random_sample(out.shape)`` -- the same doubles from NumPy's GLOBAL legacy stream, which is left where that
    call would leave it -- written into a caller-owned buffer.  (A Generator over a copy of the global MT19937 state produces the
    identical sequence; filling a reused, pinned buffer instead of a fresh 154 MB array per reference set avoids its page faults:
    0.15 -> 0.03 s per 75 000 x 256 draw, which had become the bottleneck of the K sweep.)"""
    st = np.random.get_state()
    if st[0] != 'MT19937':
        out[...] = np.random.random_sample(out.shape)
        return out
    bg = np.random.MT19937()
    bg.state = {'bit_generator': 'MT19937', 'state': {'key': st[1], 'pos': st[2]}}
    np.random.Generator(bg).random(out=out)
    ns = bg.state['state']
    np.random.set_state(('MT19937', ns['key'], ns['pos'], st[3], st[4]))
    return out


def _random_state_at(state):
    rs = np.random.RandomState()
    rs.set_state(state)
    return rs


class _StreamWalker:
    """Walks NumPy's global stream through the gap statistic's draws in upstream's order on a worker thread (see
    ``KM.compute_gap_internal_metric``).  Iterating yields, for the problems of this rank only and in stream order,
    ``(k index, i, buffer, state)``: ``i < n_references`` is a reference fit (``buffer`` = its uniform draws, to be handed back with
    ``release``), ``i == n_references`` the fit on the data (``buffer`` None); ``state`` is the global stream's state where that fit's
    seeding starts.  Problems of other ranks only advance the stream (their uniform draws go to a scratch buffer)."""

    def __init__(self, shape, ks, n_references, n_init, rank=0, world=1, n_buffers=2):
        self.free = queue.Queue()
        for _ in range(n_buffers):
            self.free.put(torch.empty(shape, dtype=torch.float64, pin_memory=torch.cuda.is_available()).numpy())
        self.out = queue.Queue()
        self.shape, self.ks, self.n_ref, self.n_init, self.rank, self.world = tuple(shape), ks, n_references, n_init, rank, world
        self.stop = threading.Event()           # set by the consumer when it gives up: the walker must not keep moving the GLOBAL stream
        self.thread = threading.Thread(target=self._walk, daemon=True)
        self.thread.start()

    def _walk(self):
        try:
            scratch = None
            j = 0
            for ki, k in enumerate(self.ks):
                n_seed = seed_draw_count(k, self.n_init)
                for i in range(self.n_ref + 1):
                    if self.stop.is_set():
                        return
                    mine = j % self.world == self.rank
                    j += 1
                    buf = None
                    if i < self.n_ref:
                        if mine:
                            buf = None
                            while buf is None and not self.stop.is_set():        # (a consumer that raised never releases a buffer)
                                try:
                                    buf = self.free.get(timeout=0.2)
                                except queue.Empty:
                                    pass
                            if buf is None:
                                return
                        else:
                            buf = scratch = np.empty(self.shape, np.float64) if scratch is None else scratch
                        global_uniform_into(buf)
                    state = np.random.get_state()
                    np.random.random_sample(n_seed)               # what the fit's k-means++ seeding consumes
                    if mine:
                        self.out.put((ki, i, buf, state))
            self.out.put(None)
        except BaseException as e:                                # surfaced by the consumer
            self.out.put(e)

    def __iter__(self):
        while True:
            item = self.out.get()
            if item is None:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def release(self, buf):
        self.free.put(buf)

    def close(self):
        """Stop walking (the consumer raised or is done) and wait for the thread: nothing touches NumPy's global stream afterwards."""
        self.stop.set()
        self.thread.join()

    def join(self):
        self.thread.join()


class _Branch(object):
    """What the branch objects below share: the plot directory, the --internal_metrics of a labelling, and "my files exist and ``overwrite`` is not set:
    leave them alone and return the table on disk".  Where the branches differ in that, the difference is data: ``FILES`` (what a run writes),
    ``NAMED`` (which of them the 'Not saved for' line names), ``TABLE`` (which of them ``train`` returns) and ``ROUND_TRIP`` (how it is read back)."""
    FILES = ()
    NAMED = 0
    TABLE = 0
    ROUND_TRIP = True          # float_precision='round_trip' (repr / %.17g: exact)

    def _open(self, out_path, internal_metrics=(), metric_sample=0):
        self.out_path = osp.join(out_path, 'plot')
        os.makedirs(self.out_path, exist_ok=True)
        self.metric_sample = metric_sample
        self.internal_metrics_names = list(internal_metrics)
        self.internal_metrics = build_metrics(internal_metrics)

    def _paths(self):
        return [osp.join(self.out_path, name) for name in self.FILES]

    def _left_alone(self, overwrite, wanted=None, named=None):
        """True, and logged, where every file of ``wanted`` (default: all of ``FILES``) exists and ``overwrite`` is not set."""
        paths = self._paths()
        if overwrite or not all(osp.exists(f) for f in (paths if wanted is None else wanted)):
            return False
        logger.info('Not saved for {}! Because files existed and not allowed for overwrite.'.format(paths[self.NAMED] if named is None else named))
        return True

    def _table_on_disk(self):
        """The table an earlier run wrote; None where it wrote none (only Optics leaves its files alone without looking for the table)."""
        f = self._paths()[self.TABLE]
        if not osp.exists(f):
            return None
        return pd.read_csv(f, float_precision='round_trip') if self.ROUND_TRIP else pd.read_csv(f)

    def _metric_values(self, Xd, labels, **kwargs):
        return metric_values(Xd, labels, self.internal_metrics, self.metric_sample, **kwargs)

    def _metric_log(self, vals):
        return metric_log(self.internal_metrics_names, vals)


class KM(_Branch):
    def __init__(self, k_max, out_path, internal_metrics, n_init, gap_b, metric_sample=0):
        self.k_max, self.n_init, self.gap_b = k_max, n_init, gap_b
        self._open(out_path, internal_metrics, metric_sample)

    # -- inertia definitions of the gap statistic (p2:334-351): one tiled pair pass on the device, nothing n x n
    def compute_inertia_v1(self, a, X, stats=None):
        return cluster_stats.inertia_v1(X, a, stats)

    def computer_intertia_v2(self, a, X, stats=None):
        return cluster_stats.inertia_v2(X, a, stats)

    def elbow(self, train_feat, valid_feat):
        rows = []
        dev = torch.device('cuda')
        tr, va = torch.as_tensor(train_feat, device=dev), torch.as_tensor(valid_feat, device=dev)
        for k in range(2, self.k_max + 1):
            logger.info('Running K: {}'.format(k))
            km = KMeans(n_clusters=k, init='k-means++').fit(tr)                  # n_init='auto' -> 1, as sklearn >= 1.4
            # mean distance to the nearest centre (p2:253-270's cdist(...).min(1).mean()) from the E-step kernel: no N x K matrix, no library GEMM
            rows.append(dict(k=k, train=float(km.nearest_distance(tr).mean()), valid=float(km.nearest_distance(va).mean())))
        df = pd.DataFrame(rows)
        if dist.rank() == 0:
            df.to_csv(osp.join(self.out_path, 'elbow.csv'), index=False)
        return df

    @staticmethod
    def _staged(walker, dev, lo, rng_):
        """The walker's items with every reference set already on its way to the device: ``(k index, i, reference set (N, D) f32 on the device or None, state)``.
        The upload of the NEXT set (pinned buffer -> device, scale / shift in f64 as upstream, f32 cast) is issued on a side stream before the fits of the
        current one are queued, so the 154 MB transfer (3 ms of an otherwise idle GPU per set, 190 sets per sweep) runs under them; the pinned buffer goes
        back to the walker as soon as its upload has finished."""
        side = torch.cuda.Stream(device=dev)
        it = iter(walker)

        def stage(item):
            if item is None:
                return None
            ki, i, buf, state = item
            if buf is None:
                return ki, i, None, state, None
            with torch.cuda.stream(side):
                refd = torch.as_tensor(buf).to(dev, non_blocking=True).mul_(rng_).add_(lo).float()
                done = torch.cuda.Event()
                done.record(side)
            return ki, i, refd, state, (done, buf)

        nxt = stage(next(it, None))
        while nxt is not None:
            ki, i, refd, state, pending = nxt
            if pending is not None:
                done, buf = pending
                done.synchronize()                                   # (issued a whole fit ago)
                walker.release(buf)                                  # the walker refills it for a later set
                torch.cuda.current_stream().wait_event(done)
                refd.record_stream(torch.cuda.current_stream())      # allocated on the side stream, consumed on this one
            nxt = stage(next(it, None))
            yield ki, i, refd, state

    def _fit_problems(self, walker, table, ks, n_references, Xd, lo, rng_, dev, inertia, need_minmax):
        """The fits of this rank's (K, reference set) problems, in stream order (see compute_gap_internal_metric)."""
        for ki, i, refd, state in self._staged(walker, dev, lo, rng_):
            k = ks[ki]
            km = KMeans(n_clusters=k, n_init=self.n_init, random_state=_random_state_at(state))
            # the walker skipped seed_draw_count(k, n_init) doubles for this fit WITHOUT running it: only right for k-means++ seeding with
            # exactly that many restarts
            if km.init != 'k-means++' or km._resolve_n_init(False) != walker.n_init:
                raise RuntimeError(f'gap statistic: the stream walk assumes k-means++ seeding with n_init={walker.n_init}, got init={km.init!r}, '
                                   f'n_init={km._resolve_n_init(False)}')
            if i < n_references:
                table[ki, i] = np.log(inertia(km.fit_predict(refd), refd))
                continue
            assignments = km.fit_predict(Xd)
            stats = cluster_stats.pair_stats(Xd, assignments, need_min=need_minmax, need_max=need_minmax)
            table[ki, n_references] = np.log(inertia(assignments, Xd, stats))      # the same pair pass feeds the gap term and every index
            table[ki, n_references + 1:] = self._metric_values(Xd, assignments, stats=stats)
        return table

    def compute_gap_internal_metric(self, data, k_max=5, n_references=5, version=1):
        """Gap statistic (p2:353-410): uniform reference sets over the data's bounding range, NumPy global RNG.

        Upstream's draw order on the global stream is  draw(ref_1) seeds(fit_1) draw(ref_2) ... seeds(fit on the data)  for K = 2, 3, ...
        A fit draws all its k-means++ randomness before its first distance (``kmeans.seed_draw_count`` doubles: data-independent), so
        the stream can be walked without doing any fit: ``_StreamWalker`` does that on a worker thread, handing each fit the stream state
        its seeding starts from (the fit then draws from a private ``RandomState`` in that state) and each reference fit its uniform
        draws in a pinned buffer.  The walk therefore runs ahead of the GPU work (0.03 s of host time per 75 k x 256 set), and with
        one process per GPU every rank walks the SAME stream but fits only the (K, reference set) problems it owns
        (problem j -> rank j mod world; SURVEY.md 8e: no data-path collective, one all-reduce of the result table at the end)."""
        data = np.asarray(data)
        lo, rng_ = float(data.min()), float(data.max() - data.min())
        logger.info('Data max: {}, min: {}, rng: {}'.format(data.max(), data.min(), rng_))
        dev = torch.device('cuda', torch.cuda.current_device())
        Xd = torch.as_tensor(data, dtype=torch.float32, device=dev)
        inertia = self.compute_inertia_v1 if version == 1 else self.computer_intertia_v2
        world, rank = (dist.world_size(), dist.rank()) if dist.is_sharded() else (1, 0)
        ks = list(range(2, k_max + 1))
        n_met = len(self.internal_metrics)
        # per K: [log-inertia of every reference fit | act | validity indices]; a rank fills the entries of its own problems only
        table = np.zeros((len(ks), n_references + 1 + n_met), np.float64)
        need_minmax = any(isinstance(m, DunnIndex) for m in self.internal_metrics)
        walker = _StreamWalker(data.shape, ks, n_references, KMeans(n_init=self.n_init)._resolve_n_init(False), rank, world)
        try:
            table = self._fit_problems(walker, table, ks, n_references, Xd, lo, rng_, dev, inertia, need_minmax)
        finally:
            walker.close()
        if world > 1 or dist.is_sharded():

            t = torch.as_tensor(table, device=dev)
            dist.all_reduce_sum_(t)                 # disjoint entries, zeros elsewhere: the sum is the assembled table (x + 0.0 is exact)
            table = t.cpu().numpy()
        rows = []
        for ki, k in enumerate(ks):
            local = table[ki, :n_references]
            ref_mean, ref_std = np.mean(local), np.std(local)
            ref_s = np.sqrt(1 + 1 / n_references) * ref_std
            act = table[ki, n_references]
            gap = ref_mean - act
            vals = list(table[ki, n_references + 1:])
            logger.info('k: {}, gap: {:.4f}, ref: {:.4f}, act: {:.4f}, ref_s: {:.4f} '.format(k, gap, ref_mean, act, ref_s)
                        + self._metric_log(vals))
            rows.append([k, gap, ref_mean, act, ref_s] + vals)
        return pd.DataFrame(rows, columns=['k', 'gap', 'ref', 'act', 'ref_s'] + list(self.internal_metrics_names))

    def train(self, train_data, valid_data, select_opt_k, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        out = {}
        for method in select_opt_k:
            if method == 'elbow':
                out['elbow'] = self.elbow(train_data['hidden'], valid_data['hidden'])
            elif method == 'gap_sts':
                csv = osp.join(self.out_path, 'gap_sts_v1.csv')
                if osp.exists(csv) and not overwrite:
                    logger.info('Load the previous gat_sts.csv')
                    out['gap_sts'] = pd.read_csv(csv)
                else:
                    df = self.compute_gap_internal_metric(train_data['hidden'], self.k_max, n_references=self.gap_b, version=1)
                    df = df.astype(float)
                    if dist.rank() == 0:
                        df.to_csv(csv, index=False)
                    out['gap_sts'] = df
        return out


class Dbscan(_Branch):
    """Dbscan.train (p2:90-168): one DBSCAN per eps of ``eps_range`` on the training latents (one counting pass for all of them), logged as upstream logs
    them; returns (and writes to plot/dbscan_eps.csv) the per-eps table.  ``select_eps == 'k_distance_graph'`` (p2:102-120) first writes the
    (min_samples - 1)-NN distance curve (plot/k_distance.csv: sample, dist) and its elbow (plot/k_distance_elbow.csv: k, elbow_x, elbow_y) and keeps them
    on ``k_distance_``; an existing k_distance.csv is left alone unless ``overwrite`` is set, as upstream leaves its plot."""
    COLUMNS = ['eps', 'n_core', 'n_clusters', 'n_noise', 'silhouette', 'denoise_silhouette']

    def __init__(self, eps_range, min_samples, out_path):
        self.eps_range = eps_range
        self.min_sample = min_samples
        self._open(out_path)
        self.k_distance_ = None

    def k_distance(self, Xd, overwrite=False):
        """p2:102-120 on the device copy of the latents: the k-distance table, its elbow, the log line."""
        k = self.min_sample - 1
        csv = osp.join(self.out_path, 'k_distance.csv')
        if self._left_alone(overwrite, [csv], csv):          # (dbscan_eps.csv itself is written by every run)
            return None
        graph = k_distance_graph(Xd, k)
        sorted_dist = graph['sorted_dist']
        logger.info('The detected elbow: x: {}, y: {}'.format(graph['elbow_x'], graph['elbow_y']))
        pd.DataFrame({'sample': np.arange(1, len(sorted_dist) + 1), 'dist': sorted_dist}).to_csv(csv, index=False, float_format='%.17g')
        pd.DataFrame({'k': [k], 'elbow_x': [graph['elbow_x']], 'elbow_y': [graph['elbow_y']]}).to_csv(
            osp.join(self.out_path, 'k_distance_elbow.csv'), index=False, float_format='%.17g')
        return graph

    def train(self, train_data, valid_data, select_eps, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        Xd = device_latents(train_data)
        if select_eps == 'k_distance_graph':
            self.k_distance_ = self.k_distance(Xd, overwrite)
        fits = dbscan_sweep(Xd, self.eps_range, self.min_sample)
        rows = []
        for eps, (labels, core) in zip(self.eps_range, fits):
            logger.info('\nRunning eps: {}'.format(eps))
            rows.append([float(eps), len(core)] + list(noise_summary(Xd, labels, len(core))))
        df = pd.DataFrame(rows, columns=self.COLUMNS)
        df.to_csv(osp.join(self.out_path, 'dbscan_eps.csv'), index=False)
        return df


def snn_default_eps(k):
    """round(k t / 10) for t = 2..8, deduplicated, inside [1, k]: p2's default --snn_eps (a starting point: not measured on the real latents)."""
    return sorted({min(k, max(1, int(round(k * t / 10.0)))) for t in range(2, 9)})


class Snn(_Branch):
    """One shared-neighbour graph of the training latents (``snn.snn_sweep``: ``k`` neighbours) labelled once per eps of ``eps_values`` at ``min_samples``,
    logged as Dbscan.train logs its fits.  Writes plot/snn_eps.csv (``COLUMNS``: Dbscan's, the silhouettes computed the same way, plus k and min_samples),
    plot/snn_similarity_hist.csv (similarity 0..k, pairs: the list entries at that similarity, the self entries and the pairs that are not mutual at 0) and
    plot/snn_labels.csv (one column eps<eps> per eps), and returns the per-eps table.  Existing files are left alone unless ``overwrite`` is set; the table
    on disk is returned then.  ``labels_`` keeps the labels per eps of the last run that computed them, ``stats_`` that run's ``snn_sweep`` stats."""
    COLUMNS = ['eps', 'n_core', 'n_clusters', 'n_noise', 'silhouette', 'denoise_silhouette', 'k', 'min_samples']
    FILES = ('snn_eps.csv', 'snn_similarity_hist.csv', 'snn_labels.csv')

    def __init__(self, k, eps_values, min_samples, out_path):
        self.k, self.eps_values, self.min_sample = int(k), [int(e) for e in eps_values], int(min_samples)
        self._open(out_path)
        self.labels_ = self.stats_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.labels_ = self.stats_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        eps_csv, hist_csv, labels_csv = self._paths()
        Xd = device_latents(train_data)
        stats = {}
        fits = snn_sweep(Xd, self.k, self.eps_values, self.min_sample, stats=stats)
        rows = []
        for eps, (labels, core, _) in zip(self.eps_values, fits):
            logger.info('\nRunning eps: {} (shared neighbours of {}), min_samples: {}'.format(eps, self.k, self.min_sample))
            rows.append([eps, len(core)] + list(noise_summary(Xd, labels, len(core))) + [self.k, self.min_sample])
        df = pd.DataFrame(rows, columns=self.COLUMNS)
        df.to_csv(eps_csv, index=False)
        pd.DataFrame({'similarity': np.arange(self.k + 1), 'pairs': stats['similarity_hist']}).to_csv(hist_csv, index=False)
        pd.DataFrame({'eps{}'.format(e): fit[0] for e, fit in zip(self.eps_values, fits)}).to_csv(labels_csv, index=False)
        logger.info('Saved for {}!.'.format(eps_csv))
        self.labels_, self.stats_ = {e: fit[0] for e, fit in zip(self.eps_values, fits)}, stats
        return df


class Optics(_Branch):
    """Optics.train (p2:171-223): one OPTICS fit of the training latents -- ``cluster_method`` 'xi' (xi = .05, min_cluster_size = min_samples) or 'dbscan'
    (eps = max_eps = inf) -- logged as upstream logs it; returns (and writes to plot/optics_<cluster_method>.csv) the one-row summary, and writes the data
    of upstream's reachability plot to plot/reachability_<cluster_method>.csv, every point included.  An existing reachability file is left alone unless
    ``overwrite`` is set, as upstream leaves its plot; the summary on disk is returned then.  The fit runs on the latents, not on the rows of their distance
    matrix (module docstring).  ``fit_`` keeps the fitted ``OPTICS`` of the last run that computed one."""
    COLUMNS = ['min_samples', 'n_clusters', 'n_noise']
    TABLE, ROUND_TRIP = 1, False

    def __init__(self, min_samples, cluster_method, out_path):
        if cluster_method not in ('xi', 'dbscan'):
            raise ValueError("cluster_method must be 'xi' or 'dbscan', got %r" % (cluster_method,))
        self.min_sample = min_samples
        self.cluster_method = cluster_method
        self.FILES = ('reachability_{}.csv'.format(cluster_method), 'optics_{}.csv'.format(cluster_method))
        self._open(out_path)
        self.fit_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fit_ = None
        plot_csv, summary_csv = self._paths()
        if self._left_alone(overwrite, [plot_csv]):          # (the reachability file alone, as upstream looks at its plot alone)
            return self._table_on_disk()
        Xd = device_latents(train_data)
        if self.cluster_method == 'xi':
            optics = OPTICS(min_samples=self.min_sample, cluster_method='xi', xi=.05, min_cluster_size=self.min_sample)
        else:
            optics = OPTICS(min_samples=self.min_sample, cluster_method='dbscan')
        optics.fit(Xd)
        labels = optics.labels_
        n_clusters_ = len(set(labels.tolist())) - (1 if -1 in labels else 0)
        n_noise_ = int(np.sum(labels == -1))
        logger.info('OPTICS with cluster_method: {}, n_clusters: {}, n_noise: {}'.format(self.cluster_method, n_clusters_, n_noise_))
        order = optics.ordering_
        pd.DataFrame({'x': np.arange(len(order)), 'sample': order, 'dist': optics.reachability_[order], 'label': labels[order]}).to_csv(
            plot_csv, index=False, float_format='%.17g')
        df = pd.DataFrame([[int(self.min_sample), n_clusters_, n_noise_]], columns=self.COLUMNS)
        df.to_csv(summary_csv, index=False)
        logger.info('Saved for {}!.'.format(plot_csv))
        self.fit_ = optics
        return df


class Hdbscan(_Branch):
    """One HDBSCAN tree of the training latents (min_samples as given) and one extraction per ``min_cluster_sizes`` entry, logged as Dbscan.train logs its
    fits.  Writes plot/hdbscan_mst.csv (x, sample, source, dist: every step of Prim's walk, %.17g), plot/hdbscan_sizes.csv (``COLUMNS``; the silhouettes as
    the DBSCAN branch computes them, empty below 2 clusters) and plot/hdbscan_labels.csv (one column mcs<size> per size), and returns the per-size table.
    Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then.  ``fit_`` keeps the fitted ``HDBSCAN`` of the last run
    that computed one, ``labels_`` its labels per size."""
    COLUMNS = ['min_cluster_size', 'n_clusters', 'n_noise', 'silhouette', 'denoise_silhouette']
    FILES = ('hdbscan_mst.csv', 'hdbscan_sizes.csv', 'hdbscan_labels.csv')
    TABLE, ROUND_TRIP = 1, False

    def __init__(self, min_samples, min_cluster_sizes, out_path):
        self.min_sample = min_samples
        self.min_cluster_sizes = [int(m) for m in min_cluster_sizes]
        self._open(out_path)
        self.fit_ = self.labels_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fit_ = self.labels_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        mst_csv, sizes_csv, labels_csv = self._paths()
        Xd = device_latents(train_data)
        fit, found = hdbscan_sizes(Xd, self.min_sample, self.min_cluster_sizes)
        order = fit.ordering_
        pd.DataFrame({'x': np.arange(len(order)), 'sample': order, 'source': fit.predecessor_[order], 'dist': fit.reachability_[order]}).to_csv(
            mst_csv, index=False, float_format='%.17g')
        rows = []
        for mcs in self.min_cluster_sizes:
            logger.info('\nRunning min_cluster_size: {}'.format(mcs))
            rows.append([mcs] + list(noise_summary(Xd, found[mcs][0])))
        df = pd.DataFrame(rows, columns=self.COLUMNS)
        df.to_csv(sizes_csv, index=False)
        pd.DataFrame({'mcs{}'.format(m): found[m][0] for m in self.min_cluster_sizes}).to_csv(labels_csv, index=False)
        logger.info('Saved for {}!.'.format(mst_csv))
        self.fit_, self.labels_ = fit, {m: found[m][0] for m in self.min_cluster_sizes}
        return df


class Ward(_Branch):
    """One Ward tree of the training latents (``ward.Ward``), cut at K = 2..``k_max``.  Per K: the labels, the height of the merge that takes K clusters to
    K - 1, the mean distance to the nearest centre on the training and the validation latents (the elbow's distortion) and the ``internal_metrics`` as
    ``KM`` computes them -- one shared pair pass per K, ``metric_sample`` honoured -- logged per K as ``KM`` logs.  Writes plot/ward_linkage.csv (Z: left,
    right, height, size, %.17g), plot/ward_k.csv (k, height, train_distortion, valid_distortion, the metrics) and plot/ward_labels.csv (columns k2..k<k_max>,
    0-based) and returns the per-K table.  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then.  ``fit_`` keeps the
    fitted ``ward.Ward`` of the last run that computed one."""
    FILES = ('ward_linkage.csv', 'ward_k.csv', 'ward_labels.csv')
    TABLE = 1

    def __init__(self, k_max, out_path, internal_metrics, metric_sample=0):
        self.ks = list(range(2, k_max + 1))
        self._open(out_path, internal_metrics, metric_sample)
        self.fit_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fit_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        linkage_csv, k_csv, labels_csv = self._paths()
        Xd, Vd = device_latents(train_data), device_latents(valid_data)
        fit = WardLinkage(ks=self.ks).fit(Xd)
        rows = []
        for k in self.ks:
            logger.info('Running K: {}'.format(k))
            labels = fit.labels_by_k_[k]
            centers = fit.cluster_centers_by_k_[k]
            train_d = float(fit.nearest_distance(Xd, centers).mean())
            valid_d = float(fit.nearest_distance(Vd, centers).mean())
            vals = self._metric_values(Xd, labels)
            logger.info('k: {}, height: {:.4f}, train: {:.4f}, valid: {:.4f} '.format(k, fit.heights_by_k_[k], train_d, valid_d) + self._metric_log(vals))
            rows.append([k, fit.heights_by_k_[k], train_d, valid_d] + vals)
        df = pd.DataFrame(rows, columns=['k', 'height', 'train_distortion', 'valid_distortion'] + self.internal_metrics_names)
        pd.DataFrame(fit.linkage_, columns=['left', 'right', 'height', 'size']).to_csv(linkage_csv, index=False, float_format='%.17g')
        df.to_csv(k_csv, index=False, float_format='%.17g')
        pd.DataFrame({'k{}'.format(k): fit.labels_by_k_[k] for k in self.ks}).to_csv(labels_csv, index=False)
        logger.info('Saved for {}!.'.format(linkage_csv))
        self.fit_ = fit
        return df


class Kmedoids(_Branch):
    """k-medoids (PAM) of the training latents for K = 2..``k_max`` (``kmedoids.kmedoids_sweep``: the planes prepared once, one BUILD of ``k_max`` whose
    prefixes start every K, SWAP per K).  Per K: TD (``inertia``), the SWAP searches, the convergence flag and the ``internal_metrics`` of the labels as the
    Ward branch computes them -- one shared pair pass per K, ``metric_sample`` honoured -- logged per K as ``KM`` logs.  Writes plot/kmedoids_k.csv,
    plot/kmedoids_labels.csv (columns k2..k<k_max>, 0-based) and plot/kmedoids_medoids.csv (k, cluster, the row of the medoid encounter in the training
    latents, its encounter id) and returns the per-K table.  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then.
    ``fits_`` keeps the {K: ``kmedoids.KMedoids``} of the last run that computed them."""
    FILES = ('kmedoids_k.csv', 'kmedoids_labels.csv', 'kmedoids_medoids.csv')
    COLUMNS = ['k', 'inertia', 'n_iter', 'converged']
    MEDOID_COLUMNS = ['k', 'cluster', 'medoid_index', 'encounter_id']

    def __init__(self, k_max, out_path, internal_metrics, metric_sample=0):
        self.ks = list(range(2, k_max + 1))
        self._open(out_path, internal_metrics, metric_sample)
        self.fits_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fits_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        k_csv, labels_csv, medoids_csv = self._paths()
        Xd = device_latents(train_data)
        fits = kmedoids_sweep(Xd, self.ks)
        ids = train_data.get('encounter_id') if hasattr(train_data, 'get') else None
        rows, medoid_rows = [], []
        for k in self.ks:
            logger.info('Running K: {}'.format(k))
            fit = fits[k]
            vals = self._metric_values(Xd, fit.labels_)
            logger.info('k: {}, inertia: {:.4f}, n_iter: {}, converged: {} '.format(k, fit.inertia_, fit.n_iter_, fit.converged_) + self._metric_log(vals))
            rows.append([k, fit.inertia_, fit.n_iter_, int(fit.converged_)] + vals)
            for slot, at in enumerate(fit.medoid_indices_):
                medoid_rows.append([k, slot, int(at), ids[int(at)] if ids is not None else ''])
        df = pd.DataFrame(rows, columns=self.COLUMNS + self.internal_metrics_names)
        df.to_csv(k_csv, index=False, float_format='%.17g')
        pd.DataFrame({'k{}'.format(k): fits[k].labels_ for k in self.ks}).to_csv(labels_csv, index=False)
        pd.DataFrame(medoid_rows, columns=self.MEDOID_COLUMNS).to_csv(medoids_csv, index=False)
        logger.info('Saved for {}!.'.format(k_csv))
        self.fits_ = fits
        return df


class Densitypeaks(_Branch):
    """Density peaks of the training latents (``density_peaks.density_peaks_sweep``: ONE device computation of rho, delta and parent, one cut per K = 2..
    ``k_max`` on the host).  Writes plot/densitypeaks_decision.csv (index, rho, delta, gamma, parent: the decision graph, every point), plot/densitypeaks_k.csv
    (k, gamma_gap, sizes -- the cluster sizes without the halo, joined by blanks --, n_halo and the ``internal_metrics`` of the labels without the halo, as the
    Ward branch computes them, ``metric_sample`` honoured) and plot/densitypeaks_labels.csv (columns k2..k<k_max>, 0-based, -1 for halo points) and returns
    the per-K table.  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then.  ``fits_`` keeps the
    {K: ``density_peaks.DensityPeaks``} of the last run that computed them."""
    FILES = ('densitypeaks_decision.csv', 'densitypeaks_k.csv', 'densitypeaks_labels.csv')
    COLUMNS = ['k', 'gamma_gap', 'sizes', 'n_halo']
    DECISION_COLUMNS = ['index', 'rho', 'delta', 'gamma', 'parent']
    NAMED = TABLE = 1

    def __init__(self, k_max, out_path, internal_metrics, density='cutoff', percent=2.0, dc=None, halo=False, metric_sample=0):
        self.ks = list(range(2, k_max + 1))
        self.kw = dict(density=density, percent=percent, dc='auto' if dc is None else dc, halo=bool(halo))
        self._open(out_path, internal_metrics, metric_sample)
        self.fits_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fits_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        decision_csv, k_csv, labels_csv = self._paths()
        Xd = device_latents(train_data)
        fits = density_peaks_sweep(Xd, self.ks, **self.kw)
        first = fits[self.ks[0]]
        rows = []
        for k in self.ks:
            logger.info('Running K: {}'.format(k))
            fit = fits[k]
            labels = fit.core_labels_
            vals = self._metric_values(Xd, labels)
            sizes = np.bincount(labels, minlength=k)
            logger.info('k: {}, gamma gap: {:.4f}, sizes: {}, halo: {} '.format(k, fit.gamma_gap_, sizes.tolist(), int(fit.halo_.sum()))
                        + self._metric_log(vals))
            rows.append([k, fit.gamma_gap_, ' '.join(str(int(v)) for v in sizes), int(fit.halo_.sum())] + vals)
        df = pd.DataFrame(rows, columns=self.COLUMNS + self.internal_metrics_names)
        pd.DataFrame({'index': np.arange(len(first.rho_)), 'rho': first.rho_, 'delta': first.delta_, 'gamma': first.gamma_,
                      'parent': first.parent_}).to_csv(decision_csv, index=False, float_format='%.17g')
        df.to_csv(k_csv, index=False, float_format='%.17g')
        pd.DataFrame({'k{}'.format(k): fits[k].labels_ for k in self.ks}).to_csv(labels_csv, index=False)
        logger.info('Saved for {}!.'.format(k_csv))
        self.fits_ = fits
        return df


class Gmm(_Branch):
    """Gaussian mixtures of the training latents (``gmm.gmm_sweep``) for K = 2..``k_max``, ``n_init`` restarts each.  Per K: the lower bound, BIC and AIC on the
    training latents, the iterations and whether the winning restart converged, the mean log-likelihood of the validation cohort under the training model, and
    the ``internal_metrics`` of the hard labels as ``KM`` computes them -- one shared pair pass per K, ``metric_sample`` honoured -- logged per K as ``KM``
    logs.  Writes plot/gmm_k.csv (k, lower_bound, bic, aic, n_iter, converged, valid_score, the metrics) and plot/gmm_labels.csv (columns k2..k<k_max>,
    0-based) and returns the per-K table.  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then.  ``fits_`` keeps the
    fitted models {K: ``gmm.GaussianMixture`` or ``gmm_full.FullGaussianMixture``} of the last run that computed them."""
    FILES = ('gmm_k.csv', 'gmm_labels.csv')

    def __init__(self, k_max, out_path, internal_metrics, n_init=1, covariance_type='diag', metric_sample=0):
        self.ks = list(range(2, k_max + 1))
        self.n_init, self.covariance_type = n_init, covariance_type
        self._open(out_path, internal_metrics, metric_sample)
        self.fits_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fits_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        k_csv, labels_csv = self._paths()
        Xd, Vd = device_latents(train_data), device_latents(valid_data)
        sweep = gmm_full_sweep if self.covariance_type in ('full', 'tied') else gmm_sweep
        fits = sweep(Xd, self.ks, covariance_type=self.covariance_type, n_init=self.n_init)
        rows = []
        for k in self.ks:
            logger.info('Running K: {}'.format(k))
            fit = fits[k]
            labels = np.unique(fit.labels_, return_inverse=True)[1].astype(np.int64)          # (a component without a row of its own is skipped by the indices)
            bic, aic, valid = float(fit.bic(Xd)), float(fit.aic(Xd)), float(fit.score(Vd))
            vals = self._metric_values(Xd, labels, nan_below_two=True)
            logger.info('k: {}, lower_bound: {:.4f}, bic: {:.1f}, aic: {:.1f}, n_iter: {}, valid: {:.4f} '.format(k, fit.lower_bound_, bic, aic, fit.n_iter_,
                                                                                                                valid)
                        + self._metric_log(vals))
            rows.append([k, fit.lower_bound_, bic, aic, fit.n_iter_, int(fit.converged_), valid] + vals)
        df = pd.DataFrame(rows, columns=['k', 'lower_bound', 'bic', 'aic', 'n_iter', 'converged', 'valid_score'] + self.internal_metrics_names)
        df.to_csv(k_csv, index=False, float_format='%.17g')
        pd.DataFrame({'k{}'.format(k): fits[k].labels_ for k in self.ks}).to_csv(labels_csv, index=False)
        logger.info('Saved for {}!.'.format(k_csv))
        self.fits_ = fits
        return df


class Fcm(_Branch):
    """Fuzzy c-means of the training latents (``fcm.fcm_sweep``), one sweep per fuzzifier of ``ms`` over K = 2..``k_max``, ``n_init`` restarts each.  Per
    (m, K): the objective, the partition coefficient, its modified form, the partition entropy, Xie-Beni and the fuzzy silhouette of the training latents, the
    iterations and whether the winning restart converged, the number of coincident centre pairs (non-zero: the fit collapsed), the partition coefficient
    of the validation cohort under the training centres, and the ``internal_metrics`` of the hard labels as ``Gmm`` computes them.  Writes plot/fcm_k.csv
    (``COLUMNS``, the metrics), plot/fcm_labels.csv (columns m<m>_k<K>, 0-based) and plot/fcm_centers.csv (m, k, cluster, x0, x1, ..), %.17g, and returns
    the first table.  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then.  ``fits_`` keeps the fitted models
    {(m, K): ``fcm.FuzzyCMeans``} of the last run that computed them."""
    FILES = ('fcm_k.csv', 'fcm_labels.csv', 'fcm_centers.csv')
    COLUMNS = ['m', 'k', 'objective', 'partition_coefficient', 'modified_partition_coefficient', 'partition_entropy', 'xie_beni', 'fuzzy_silhouette',
               'n_iter', 'converged', 'n_coincident', 'valid_partition_coefficient']

    def __init__(self, k_max, out_path, internal_metrics, n_init=1, ms=(2.0,), metric_sample=0):
        self.ks = list(range(2, k_max + 1))
        self.n_init, self.ms = n_init, [float(m) for m in ms]
        self._open(out_path, internal_metrics, metric_sample)
        self.fits_ = None

    @staticmethod
    def column(m, k):
        return 'm{:g}_k{}'.format(m, k)

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fits_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        k_csv, labels_csv, centers_csv = self._paths()
        Xd, Vd = device_latents(train_data), device_latents(valid_data)
        fits, rows, columns, centers = {}, [], {}, []
        for m in self.ms:
            logger.info('Running m: {:g}'.format(m))
            with warnings.catch_warnings(record=True) as caught:          # (a collapsed fit is a row of the table here, and one log line)
                warnings.simplefilter('always')
                by_k = fcm_sweep(Xd, self.ks, m=m, n_init=self.n_init)
            for w in caught:
                logger.info(str(w.message))
            for k in self.ks:
                logger.info('Running K: {}'.format(k))
                fit = fits[(m, k)] = by_k[k]
                labels = np.unique(fit.labels_, return_inverse=True)[1].astype(np.int64)          # (a centre without a row of its own is skipped by the indices)
                fs = float(fit.fuzzy_silhouette(Xd))
                u = fit.memberships(Vd)
                valid_pc = float((u * u).sum() / len(u))
                vals = self._metric_values(Xd, labels, nan_below_two=True)
                logger.info('m: {:g}, k: {}, objective: {:.4f}, PC: {:.4f}, PE: {:.4f}, XB: {:.4f}, FS: {:.4f}, n_iter: {}, coincident: {}, valid PC: {:.4f} '.format(
                    m, k, fit.objective_, fit.partition_coefficient_, fit.partition_entropy_, fit.xie_beni_, fs, fit.n_iter_, len(fit.coincident_centers_),
                    valid_pc) + self._metric_log(vals))
                rows.append([m, k, fit.objective_, fit.partition_coefficient_, fit.modified_partition_coefficient_, fit.partition_entropy_, fit.xie_beni_, fs,
                             fit.n_iter_, int(fit.converged_), len(fit.coincident_centers_), valid_pc] + vals)
                columns[self.column(m, k)] = fit.labels_
                centers.append(np.column_stack([np.full(k, m), np.full(k, k), np.arange(k), fit.cluster_centers_]))
        df = pd.DataFrame(rows, columns=self.COLUMNS + self.internal_metrics_names)
        df.to_csv(k_csv, index=False, float_format='%.17g')
        pd.DataFrame(columns).to_csv(labels_csv, index=False)
        width = centers[0].shape[1] - 3
        pd.DataFrame(np.concatenate(centers), columns=['m', 'k', 'cluster'] + ['x{}'.format(c) for c in range(width)]).astype(
            {'k': np.int64, 'cluster': np.int64}).to_csv(centers_csv, index=False, float_format='%.17g')
        logger.info('Saved for {}!.'.format(k_csv))
        self.fits_ = fits
        return df


class Bgmm(_Branch):
    """Bayesian Gaussian mixtures of the training latents (``bgmm.bgmm_sweep``) with ``k_max`` components, one fit per weight concentration prior of
    ``concentrations`` (default 1 / k_max), ``n_init`` restarts each.  Per concentration: the components that are some training row's label (active), the
    lower bound, the iterations and whether the winning restart converged, the mean log-likelihood of the validation cohort under the training model, and
    the ``internal_metrics`` of the hard labels as ``Gmm`` computes them.  Writes plot/bgmm_k.csv (concentration, n_components, n_active, lower_bound,
    n_iter, converged, valid_score, the metrics), plot/bgmm_weights.csv (concentration, component, weight, n_k, mean_precision, degrees_of_freedom,
    active: one row per component and fit) and plot/bgmm_labels.csv (columns c0, c1, .. in the table's order: the active components renumbered 0..A-1 in
    ascending component order) and returns the first table.  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned
    then.  ``fits_`` keeps the fitted models [``bgmm.BayesianGaussianMixture``] of the last run that computed them, in the table's order."""
    FILES = ('bgmm_k.csv', 'bgmm_weights.csv', 'bgmm_labels.csv')
    COLUMNS = ['concentration', 'n_components', 'n_active', 'lower_bound', 'n_iter', 'converged', 'valid_score']
    WEIGHT_COLUMNS = ['concentration', 'component', 'weight', 'n_k', 'mean_precision', 'degrees_of_freedom', 'active']

    def __init__(self, k_max, out_path, internal_metrics, n_init=1, covariance_type='diag', concentrations=None, prior_type='dirichlet_process',
                 metric_sample=0):
        self.k_max, self.n_init, self.covariance_type, self.prior_type = k_max, n_init, covariance_type, prior_type
        self.concentrations = [1.0 / k_max] if concentrations is None else [float(c) for c in concentrations]
        self._open(out_path, internal_metrics, metric_sample)
        self.fits_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fits_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        k_csv, weights_csv, labels_csv = self._paths()
        Xd, Vd = device_latents(train_data), device_latents(valid_data)
        by_c = bgmm_sweep(Xd, sorted(set(self.concentrations)), n_components=self.k_max, covariance_type=self.covariance_type, n_init=self.n_init,
                          weight_concentration_prior_type=self.prior_type)
        fits = [by_c[c] for c in self.concentrations]
        rows, weight_rows, columns = [], [], {}
        for i, (c, fit) in enumerate(zip(self.concentrations, fits)):
            logger.info('Running concentration: {:.6g}'.format(c))
            active = fit.active_components_
            labels = np.searchsorted(active, fit.labels_).astype(np.int64)          # (active components -> 0..A-1, ascending)
            valid = float(fit.score(Vd))
            vals = self._metric_values(Xd, labels, nan_below_two=True)
            logger.info('concentration: {:.6g}, active: {} of {}, lower_bound: {:.4f}, n_iter: {}, valid: {:.4f} '.format(
                c, len(active), self.k_max, fit.lower_bound_, fit.n_iter_, valid) + self._metric_log(vals))
            rows.append([c, self.k_max, len(active), fit.lower_bound_, fit.n_iter_, int(fit.converged_), valid] + vals)
            nk = fit.degrees_of_freedom_ - fit.degrees_of_freedom_prior_          # (nu_k = nu0 + n_k)
            for k in range(self.k_max):
                weight_rows.append([c, k, fit.weights_[k], nk[k], fit.mean_precision_[k], fit.degrees_of_freedom_[k], int(k in active)])
            columns['c{}'.format(i)] = labels
        df = pd.DataFrame(rows, columns=self.COLUMNS + self.internal_metrics_names)
        df.to_csv(k_csv, index=False, float_format='%.17g')
        pd.DataFrame(weight_rows, columns=self.WEIGHT_COLUMNS).to_csv(weights_csv, index=False, float_format='%.17g')
        pd.DataFrame(columns).to_csv(labels_csv, index=False)
        logger.info('Saved for {}!.'.format(k_csv))
        self.fits_ = fits
        return df


class Meanshift(_Branch):
    """Mean shift of the training latents (``meanshift.mean_shift_sweep``), one fit per bandwidth: the given ``bandwidths``, or ``estimate_bandwidth`` of the
    training latents at every quantile of ``quantiles``.  Per bandwidth: the clusters found, the orphans (``cluster_all`` off), the largest and the smallest
    cluster, the iterations, the validation cohort's mean distance to its nearest centre (``predict``) and the ``internal_metrics`` of the labels as ``KM``
    computes them (orphans left out) -- one shared pair pass, ``metric_sample`` honoured -- logged per fit.  Writes plot/meanshift_bandwidth.csv,
    plot/meanshift_labels.csv (columns bw0, bw1, .. in the table's order) and plot/meanshift_centers.csv (bandwidth, cluster, x0, x1, ..), all %.17g, and
    returns the table.  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then.  ``fits_`` keeps the fitted models
    [``meanshift.MeanShift``] of the last run that computed them, in the table's order."""
    FILES = ('meanshift_bandwidth.csv', 'meanshift_labels.csv', 'meanshift_centers.csv')
    COLUMNS = ['quantile', 'bandwidth', 'n_clusters', 'n_orphans', 'largest', 'smallest', 'n_iter', 'valid_distortion']

    def __init__(self, out_path, internal_metrics, quantiles=(0.1, 0.2, 0.3), bandwidths=None, bin_seeding=False, cluster_all=True, metric_sample=0):
        self.quantiles, self.bandwidths = list(quantiles), None if bandwidths is None else [float(b) for b in bandwidths]
        self.bin_seeding, self.cluster_all = bool(bin_seeding), bool(cluster_all)
        self._open(out_path, internal_metrics, metric_sample)
        self.fits_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fits_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        bw_csv, labels_csv, centers_csv = self._paths()
        Xd, Vd = device_latents(train_data), device_latents(valid_data)
        if self.bandwidths is not None:
            plan = [(float('nan'), b) for b in self.bandwidths]
        else:
            plan = [(q, estimate_bandwidth(Xd, q)) for q in self.quantiles]
        by_bw = mean_shift_sweep(Xd, sorted(set(b for _, b in plan)), bin_seeding=self.bin_seeding, cluster_all=self.cluster_all)
        fits = [by_bw[b] for _, b in plan]
        rows = []
        for (q, b), fit in zip(plan, fits):
            logger.info('Running bandwidth: {:.6g} (quantile {})'.format(b, q))
            keep = fit.labels_ >= 0
            sizes = np.bincount(fit.labels_[keep], minlength=len(fit.cluster_centers_))
            cv = fit.cluster_centers_[fit.predict(Vd)]
            valid_d = float(np.sqrt(((np.asarray(valid_data['hidden'], dtype=np.float64) - cv) ** 2).sum(axis=1)).mean())
            labels = np.unique(fit.labels_[keep], return_inverse=True)[1].astype(np.int64)
            Xk = Xd if keep.all() else Xd[torch.as_tensor(keep, device=Xd.device)]
            vals = self._metric_values(Xk, labels, nan_below_two=True)          # (the subsample is drawn from the points that are no orphans)
            row = [q, b, len(fit.cluster_centers_), int((~keep).sum()), int(sizes.max()), int(sizes.min()), fit.n_iter_, valid_d]
            logger.info('bandwidth: {:.6g}, clusters: {}, orphans: {}, largest: {}, smallest: {}, n_iter: {}, valid: {:.4f} '.format(*row[1:])
                        + self._metric_log(vals))
            rows.append(row + vals)
        df = pd.DataFrame(rows, columns=self.COLUMNS + self.internal_metrics_names)
        df.to_csv(bw_csv, index=False, float_format='%.17g')
        pd.DataFrame({'bw{}'.format(i): fit.labels_ for i, fit in enumerate(fits)}).to_csv(labels_csv, index=False)
        width = fits[0].cluster_centers_.shape[1]
        cen = [np.column_stack([np.full(len(f.cluster_centers_), b), np.arange(len(f.cluster_centers_)), f.cluster_centers_]) for (_, b), f in zip(plan, fits)]
        pd.DataFrame(np.concatenate(cen), columns=['bandwidth', 'cluster'] + ['x{}'.format(c) for c in range(width)]).astype({'cluster': np.int64}).to_csv(
            centers_csv, index=False, float_format='%.17g')
        logger.info('Saved for {}!.'.format(bw_csv))
        self.fits_ = fits
        return df


class Spectral(_Branch):
    """One spectral decomposition of the training latents (``spectral.spectral_sweep``: ``k`` neighbours, k_max + 1 eigenpairs) labelled for K = 2..``k_max``
    from the first K eigenvectors.  Per K: the eigengap theta_K - theta_(K+1), the solver's iterations and whether it converged, the number of connected
    components and the ``internal_metrics`` of the labels on the latents as ``KM`` computes them -- one shared pair pass per K, ``metric_sample`` honoured.
    Writes plot/spectral_eigenvalues.csv (index 1..k_max + 1, eigenvalue, eigengap: the gap to the next eigenvalue, NaN for the last), plot/spectral_k.csv and
    plot/spectral_labels.csv (columns k2..k<k_max>, 0-based) and returns the per-K table.  Existing files are left alone unless ``overwrite`` is set; the
    table on disk is returned then.  ``fit_`` keeps the fitted ``spectral.SpectralClustering`` of the last run that computed one."""
    FILES = ('spectral_eigenvalues.csv', 'spectral_k.csv', 'spectral_labels.csv')
    NAMED = TABLE = 1

    def __init__(self, k_max, out_path, internal_metrics, k=10, assign_labels='kmeans', metric_sample=0):
        if not 2 <= k_max <= MAX_CLUSTERS - 1:
            raise ValueError('--cluster_method spectral: --k_max must lie in [2, {}] (k_max + 1 eigenpairs are computed, for the gap after the last K, and '
                             '{} is the compiled limit), got {}'.format(MAX_CLUSTERS - 1, MAX_CLUSTERS, k_max))
        self.ks = list(range(2, k_max + 1))
        self.k, self.assign_labels = k, assign_labels
        self._open(out_path, internal_metrics, metric_sample)
        self.fit_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fit_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        eig_csv, k_csv, labels_csv = self._paths()
        Xd = device_latents(train_data)
        fit = spectral_sweep(Xd, self.ks, n_neighbors=self.k, assign_labels=self.assign_labels, random_state=0, n_components=self.ks[-1] + 1,
                             return_fit=True)
        theta = fit.eigenvalues_
        gaps = np.append(theta[:-1] - theta[1:], np.nan)
        rows = []
        for k in self.ks:
            logger.info('Running K: {}'.format(k))
            labels = np.unique(fit.labels_by_k_[k], return_inverse=True)[1].astype(np.int64)          # (an empty cluster is skipped by the indices)
            vals = self._metric_values(Xd, labels, nan_below_two=True)
            logger.info('k: {}, eigengap: {:.6f}, n_iter: {}, components: {} '.format(k, gaps[k - 1], fit.n_iter_, fit.n_connected_components_)
                        + self._metric_log(vals))
            rows.append([k, gaps[k - 1], fit.n_iter_, int(fit.converged_), fit.n_connected_components_] + vals)
        df = pd.DataFrame(rows, columns=['k', 'eigengap', 'n_iter', 'converged', 'n_connected_components'] + self.internal_metrics_names)
        pd.DataFrame({'index': np.arange(1, len(theta) + 1), 'eigenvalue': theta, 'eigengap': gaps}).to_csv(eig_csv, index=False, float_format='%.17g')
        df.to_csv(k_csv, index=False, float_format='%.17g')
        pd.DataFrame({'k{}'.format(k): fit.labels_by_k_[k] for k in self.ks}).to_csv(labels_csv, index=False)
        logger.info('Saved for {}!.'.format(k_csv))
        self.fit_ = fit
        return df


class Tsne(_Branch):
    """--embed tsne: one exact t-SNE fit of the training latents (``tsne.TSNE``: init 'pca', ``perplexity``, ``max_iter`` iterations).  Writes plot/tsne.csv
    (x, y as %.17g, one row per training encounter in the cohort's row order -- the order of every plot/*_labels.csv) and plot/tsne_kl.csv (iteration, kl:
    the error at every check, every 50 iterations, and at the last iteration) and returns the latter table.  Existing files are left alone unless
    ``overwrite`` is set; the table on disk is returned then.  ``fit_`` keeps the fitted ``TSNE`` of the last run that computed one.  ``quality_k`` (a list
    of neighbourhood sizes, --embed_quality_k): also plot/tsne_quality.csv (k, trustworthiness, continuity, neighbors_kept as %.17g) from ``fit.quality``;
    without it that file is neither written nor looked for."""
    FILES = ('tsne.csv', 'tsne_kl.csv')
    QUALITY_FILE = 'tsne_quality.csv'
    TABLE = 1

    def __init__(self, out_path, perplexity=30.0, max_iter=1000, quality_k=None):
        self.perplexity, self.max_iter = perplexity, max_iter
        self.quality_k = [int(k) for k in quality_k] if quality_k else None
        self._open(out_path)
        self.fit_ = None

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fit_ = None
        map_csv, kl_csv = self._paths()
        quality_csv = osp.join(self.out_path, self.QUALITY_FILE)
        if self._left_alone(overwrite, [map_csv, kl_csv] + ([quality_csv] if self.quality_k else [])):
            return self._table_on_disk()
        fit = TSNE(perplexity=self.perplexity, max_iter=self.max_iter, init='pca').fit(device_latents(train_data))
        logger.info('t-SNE with perplexity: {}, n_iter: {}, kl: {:.6f}'.format(self.perplexity, fit.n_iter_, fit.kl_divergence_))
        pd.DataFrame({'x': fit.embedding_[:, 0], 'y': fit.embedding_[:, 1]}).to_csv(map_csv, index=False, float_format='%.17g')
        df = pd.DataFrame(fit.kl_history_, columns=['iteration', 'kl'])
        df.to_csv(kl_csv, index=False, float_format='%.17g')
        if self.quality_k:
            quality = fit.quality(self.quality_k)
            pd.DataFrame([(k,) + quality[k] for k in sorted(quality)], columns=['k', 'trustworthiness', 'continuity', 'neighbors_kept']).to_csv(
                quality_csv, index=False, float_format='%.17g')
            for k in sorted(quality):
                logger.info('t-SNE map at k: {}, trustworthiness: {:.6f}, continuity: {:.6f}, neighbors kept: {:.6f}'.format(k, *quality[k]))
        logger.info('Saved for {}!.'.format(map_csv))
        self.fit_ = fit
        return df


class Lof(_Branch):
    """--outlier lof: the local outlier factor of the training latents at every k of ``ks`` from one neighbour join (``lof.LofSweep``).  Writes
    plot/lof.csv (per k ``lof_k<k>`` = -negative_outlier_factor_ as %.17g and ``outlier_k<k>`` = 0 / 1, then ``lof_max``; one row per training encounter in
    the cohort's row order) and plot/lof_summary.csv (k, offset, n_outliers, max_lof) and returns the latter table.  Existing files are left alone unless
    ``overwrite`` is set; the table on disk is returned then.  ``fit_`` keeps the ``LofSweep`` of the last run that computed one."""
    FILES = ('lof.csv', 'lof_summary.csv')
    TABLE = 1

    def __init__(self, out_path, ks=(20,), contamination='auto'):
        self.ks = sorted(set(int(k) for k in ks))
        self.contamination = contamination
        self._open(out_path)
        self.fit_ = None

    def train(self, train_data, valid_data, **kwargs):
        from .lof import LofSweep          # (here, not at module scope: a run without --outlier loads nothing of it)
        overwrite = kwargs.get('overwrite', False)
        self.fit_ = None
        if self._left_alone(overwrite):
            return self._table_on_disk()
        lof_csv, summary_csv = self._paths()
        fit = LofSweep(device_latents(train_data), self.ks, contamination=self.contamination)
        columns = {}
        for t, k in enumerate(self.ks):
            columns['lof_k{}'.format(k)] = -fit.nof[:, t]
            columns['outlier_k{}'.format(k)] = (fit.nof[:, t] < fit.offsets[t]).astype(np.int64)
        columns['lof_max'] = (-fit.nof).max(axis=1)
        pd.DataFrame(columns).to_csv(lof_csv, index=False, float_format='%.17g')
        df = pd.DataFrame({'k': self.ks, 'offset': fit.offsets, 'n_outliers': [int(columns['outlier_k{}'.format(k)].sum()) for k in self.ks],
                           'max_lof': [float(columns['lof_k{}'.format(k)].max()) for k in self.ks]})
        df.to_csv(summary_csv, index=False, float_format='%.17g')
        for row in df.itertuples(index=False):
            logger.info('LOF at k: {}, offset: {:.6f}, outliers: {}, max factor: {:.6f}'.format(row.k, row.offset, row.n_outliers, row.max_lof))
        logger.info('Saved for {}!.'.format(lof_csv))
        self.fit_ = fit
        return df


class Dbcv(_Branch):
    """--validity dbcv: the DBCV (dbcv.py) of every column of the method's plot/<method>_labels.csv on the training latents, after the branch has run.
    Writes plot/dbcv.csv (labelling, n_clusters, n_noise, n_singletons, dbcv: one row per column, NaN below two clusters) and plot/dbcv_clusters.csv
    (labelling, cluster, size, sparseness, separation, nearest_cluster, validity), %.17g, and returns the former table.  A method that writes no such
    label file is logged and skipped (None).  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then."""
    FILES = ('dbcv.csv', 'dbcv_clusters.csv')

    def __init__(self, out_path, method):
        self.method = method
        self._open(out_path)

    def train(self, train_data, valid_data, **kwargs):
        labels_csv = osp.join(self.out_path, '{}_labels.csv'.format(self.method))
        if not osp.exists(labels_csv):
            logger.info('No DBCV for --cluster_method {}: it writes no {}.'.format(self.method, labels_csv))
            return None
        if self._left_alone(kwargs.get('overwrite', False)):
            return self._table_on_disk()
        table_csv, clusters_csv = self._paths()
        labels = pd.read_csv(labels_csv)
        rows, cluster_rows = dbcv_summary(device_latents(train_data), {name: labels[name].to_numpy() for name in labels.columns})
        df = pd.DataFrame(rows, columns=DBCV_COLUMNS)
        df.to_csv(table_csv, index=False, float_format='%.17g')
        pd.DataFrame(cluster_rows, columns=DBCV_CLUSTER_COLUMNS).to_csv(clusters_csv, index=False, float_format='%.17g')
        logger.info('Saved for {}!.'.format(table_csv))
        return df


class Agreement(_Branch):
    """--agreement: the training labellings on disk compared with each other (agreement.py), after the branch and --validity have run.  ``scope`` 'method':
    the columns of this run's plot/<method>_labels.csv; 'all': those of every method's label file under the same out_feat directory and of the training
    consensus labels (``training_labellings``).  Writes plot/agreement.csv (one row per unordered pair: labelling_a, labelling_b, n, clusters_a, clusters_b,
    then the indices) and one square plot/agreement_<index>.csv per index (the names as header and first column), %.17g, and returns the former table.
    Fewer than two labellings: logged, nothing written (None).  Existing files are left alone unless ``overwrite`` is set; the table on disk is returned then."""

    def __init__(self, out_path, method, indices, scope='all', noise='class'):
        self.method, self.indices, self.scope, self.noise = method, list(dict.fromkeys(indices)), scope, noise
        self.FILES = ('agreement.csv',) + tuple('agreement_{}.csv'.format(name) for name in self.indices)
        self.metric = osp.basename(out_path)[:-len('_{}_aligned'.format(method))]
        self.out_feat = osp.dirname(out_path)
        self._open(out_path)

    def train(self, train_data, valid_data, **kwargs):
        if self._left_alone(kwargs.get('overwrite', False)):
            return self._table_on_disk()
        everything = self.scope == 'all'
        labellings = training_labellings(self.out_feat, self.metric, METHODS if everything else [self.method], len(train_data['encounter_id']), everything)
        if len(labellings) < 2:
            logger.info('No agreement: {} labelling of the training cohort on disk, two are needed.'.format(len(labellings)))
            return None
        rows, squares = agreement_summary(labellings, self.indices, self.noise)
        paths = self._paths()
        df = pd.DataFrame(rows, columns=AGREEMENT_COLUMNS + self.indices)
        df.to_csv(paths[0], index=False, float_format='%.17g')
        for name, f in zip(self.indices, paths[1:]):
            pd.DataFrame(squares[name], index=list(labellings), columns=list(labellings)).to_csv(f, index_label='labelling', float_format='%.17g')
        logger.info('Saved for {}!.'.format(paths[0]))
        return df


class Consensus(_Branch):
    """Consensus clustering of the training and of the validation latents for K = 2..k_max, each cohort on its own (``consensus.ConsensusKMeans``).  Writes the
    training cohort's CDFs to plot/consensus_cdf.csv (k, c, cdf) and areas to plot/consensus_area.csv (k, area, delta_area) under ``out_path``, and the 1-based
    labels of either cohort to ``raw_path``/<cohort>_consensus.csv (columns k2..k<k_max>), the file p4's consensus branch reads.  A cohort whose files exist
    is left alone unless ``overwrite`` is set.  Returns the area table (read back from disk when it was left alone); ``fits_`` keeps the fits of this run."""

    FILES = ('consensus_cdf.csv', 'consensus_area.csv')          # (beside them: one raw label file per cohort, under ``raw_path``)
    TABLE = 1

    def __init__(self, k_max, out_path, raw_path, reps=100, p_item=0.8, n_init=1, seed=0):
        self.ks = list(range(2, k_max + 1))
        self.reps, self.p_item, self.n_init, self.seed = reps, p_item, n_init, seed
        self._open(out_path)
        self.raw_path = raw_path
        os.makedirs(self.raw_path, exist_ok=True)
        self.fits_ = {}

    def _fit(self, cohort, data):
        logger.info('Consensus clustering of the {} cohort: K = {}..{}, {} resamples'.format(cohort, self.ks[0], self.ks[-1], self.reps))
        cc = ConsensusKMeans(self.ks, reps=self.reps, p_item=self.p_item, n_init=self.n_init, seed=self.seed)
        cc.fit(device_latents(data))
        self.fits_[cohort] = cc
        return cc

    def train(self, train_data, valid_data, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        self.fits_ = {}
        cdf_csv, area_csv = self._paths()
        for cohort, data in (('training', train_data), ('validation', valid_data)):
            raw_csv = osp.join(self.raw_path, '{}_consensus.csv'.format(cohort))
            if self._left_alone(overwrite, [raw_csv] + ([cdf_csv, area_csv] if cohort == 'training' else []), raw_csv):          # (per cohort)
                continue
            cc = self._fit(cohort, data)
            pd.DataFrame({'k{}'.format(k): cc.labels_[k] for k in self.ks}).to_csv(raw_csv, index=False)
            if cohort == 'training':
                grid = np.arange(BINS + 1) / BINS
                pd.concat([pd.DataFrame({'k': k, 'c': grid, 'cdf': cc.cdf_[k]}) for k in self.ks]).to_csv(cdf_csv, index=False, float_format='%.17g')
                pd.DataFrame({'k': self.ks, 'area': [cc.area_[k] for k in self.ks], 'delta_area': [cc.delta_area_[k] for k in self.ks]}).to_csv(
                    area_csv, index=False, float_format='%.17g')
                for k in self.ks:
                    logger.info('k: {}, area: {:.5f}, delta_area: {:.5f}'.format(k, cc.area_[k], cc.delta_area_[k]))
            logger.info('Saved for {}!.'.format(raw_csv))
        return self._table_on_disk()          # (%.17g: exact)


def _snn_branch(a, d, out, tr, va):
    k = a.snn_k if a.snn_k is not None else d + 1
    return Snn(k, a.snn_eps or snn_default_eps(k), a.snn_min_samples if a.snn_min_samples is not None else k // 4, out).train(tr, va)


# --cluster_method -> build the branch object from the arguments, feat_dim and the output directory and run it on the training and the validation cohort
# (the class names are looked up when a branch runs).  A method of METHODS without an entry ('dl') raises in select_opt_k.
BRANCHES = {
    'kmeans': lambda a, d, out, tr, va: KM(a.k_max, out, a.internal_metrics, a.n_init, a.gap_b, a.metric_sample).train(tr, va, a.select_opt_k),
    'dbscan': lambda a, d, out, tr, va: Dbscan(eps_range=np.arange(.5, 5.1, .5), min_samples=d + 1, out_path=out).train(tr, va, a.select_eps),
    'optics': lambda a, d, out, tr, va: Optics(min_samples=d + 1, cluster_method='xi', out_path=out).train(tr, va),
    'consensus': lambda a, d, out, tr, va: Consensus(a.k_max, out, osp.join(osp.dirname(out), 'raw_consensus_result'), reps=a.consensus_reps,
                                                     p_item=a.consensus_p_item).train(tr, va),
    'hdbscan': lambda a, d, out, tr, va: Hdbscan(min_samples=d + 1, min_cluster_sizes=a.hdbscan_min_cluster_size or [d + 1], out_path=out).train(tr, va),
    'ward': lambda a, d, out, tr, va: Ward(a.k_max, out, a.internal_metrics, a.metric_sample).train(tr, va),
    'gmm': lambda a, d, out, tr, va: Gmm(a.k_max, out, a.internal_metrics, a.n_init, a.gmm_covariance_type, a.metric_sample).train(tr, va),
    'fcm': lambda a, d, out, tr, va: Fcm(a.k_max, out, a.internal_metrics, a.n_init, a.fcm_m, a.metric_sample).train(tr, va),
    'snn': _snn_branch,
    'spectral': lambda a, d, out, tr, va: Spectral(a.k_max, out, a.internal_metrics, a.spectral_k, a.spectral_assign, a.metric_sample).train(tr, va),
    'meanshift': lambda a, d, out, tr, va: Meanshift(out, a.internal_metrics, a.meanshift_quantile, a.meanshift_bandwidth, a.meanshift_bin_seeding,
                                                     bool(a.meanshift_cluster_all), a.metric_sample).train(tr, va),
    'kmedoids': lambda a, d, out, tr, va: Kmedoids(a.k_max, out, a.internal_metrics, a.metric_sample).train(tr, va),
    'densitypeaks': lambda a, d, out, tr, va: Densitypeaks(a.dp_k if a.dp_k is not None else a.k_max, out, a.internal_metrics, a.dp_density, a.dp_percent,
                                                           a.dp_dc, bool(a.dp_halo), a.metric_sample).train(tr, va),
    'bgmm': lambda a, d, out, tr, va: Bgmm(a.k_max, out, a.internal_metrics, a.n_init, a.gmm_covariance_type, a.bgmm_concentration, a.bgmm_prior_type,
                                           a.metric_sample).train(tr, va),
}


class Cluster(object):
    def __init__(self, args):
        self.args = args
        self.exp_path = os.path.join(os.getcwd(), 'Results', 'Pretrain')

    def load_data(self):
        cohorts = []
        for cohort in COHORTS:
            full = np.load(osp.join(self.feat_path, '{}.npy'.format(cohort)), allow_pickle=True).item()
            cohorts.append({k: full[k] for k in ['encounter_id', 'hidden', 'ob', 'padding_mask']})
            logger.info('Cohort: {}, Sample: {}'.format(cohort, len(full['encounter_id'])))
        self.train_data, self.valid_data, self.test_data = cohorts
        self.feat_dim = self.train_data['hidden'].shape[-1]

    def select_opt_k(self):
        results = {}
        for metric in self.args.restore_metric:
            self.feat_path = osp.join(self.exp_path, 'out_feat', metric)
            self.out_path = osp.join(self.exp_path, 'out_feat', '{}_{}'.format(metric, self.args.cluster_method)) + '_aligned'
            os.makedirs(self.out_path, exist_ok=True)
            self.load_data()
            if getattr(self.args, 'embed', None) == 'tsne' and dist.rank() == 0:          # (an args object from before the flag: no map)
                # one fit, on rank 0, beside whatever --cluster_method writes; it draws nothing from numpy's global stream
                Tsne(self.out_path, self.args.tsne_perplexity, self.args.tsne_max_iter, getattr(self.args, 'embed_quality_k', None)).train(self.train_data, self.valid_data)
            if getattr(self.args, 'outlier', None) == 'lof' and dist.rank() == 0:          # (an args object from before the flag: no scores)
                Lof(self.out_path, self.args.outlier_k, self.args.outlier_contamination).train(self.train_data, self.valid_data)
            run = BRANCHES.get(self.args.cluster_method)
            if run is None:
                raise NotImplementedError('only --cluster_method {} are on the accelerated path'.format(spell(m for m in METHODS if m in BRANCHES)))
            # kmeans deals its (K, reference set) problems over the ranks; every other branch is one run, on rank 0: the other ranks wait at main's barrier
            if self.args.cluster_method == 'kmeans' or dist.rank() == 0:
                results[metric] = run(self.args, self.feat_dim, self.out_path, self.train_data, self.valid_data)
            if getattr(self.args, 'validity', None) == 'dbcv' and dist.rank() == 0:          # (an args object from before the flag: no scores)
                Dbcv(self.out_path, self.args.cluster_method).train(self.train_data, self.valid_data)
            if getattr(self.args, 'agreement', None) and dist.rank() == 0:          # (an args object from before the flag: no tables)
                Agreement(self.out_path, self.args.cluster_method, self.args.agreement, getattr(self.args, 'agreement_scope', 'all'),
                          getattr(self.args, 'agreement_noise', 'class')).train(self.train_data, self.valid_data)
        return results


def main(args):
    dist.init_from_env()            # one process per GPU: the gap statistic's (K, reference set) problems are dealt over the ranks
    out = Cluster(args).select_opt_k()
    dist.barrier()
    return out


if __name__ == '__main__':
    _args = get_arguments()
    print_dict_byline(vars(_args))
    main(_args)
