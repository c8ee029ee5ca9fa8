"""p4: final cluster labels for every cohort (p4_clustering_final.py:30-313).

``kmeans``: KMeans(k, n_init=20) on the training latents (HIP kernels), clusters re-numbered by descending mean
systolic pressure so ids are comparable across runs (generate_align_map, p4:63-98), then ``predict`` on each cohort.
``dl``: argmax of the network's own soft assignment.  Reads Results/Clustering/out_feat/<metric>/<cohort>.npy,
writes .../<metric>_<method>_aligned/<cohort>_<k>.npy with an added ``cluster_id``.
``dbscan`` (p4:181-236): a DBSCAN(opt_eps, min_samples = feat_dim) fit per cohort on the GPU (dbscan.py), training clusters re-numbered by
sbp (generate_align_map), validation / test clusters mapped onto the nearest training centre (align_labels_with_center); writes
<cohort>_eps-<opt_eps>.npy.  ``optics`` is accepted by the parser but does nothing upstream (its branch is ``pass``, p4:238-239), so there is nothing to
provide here: it raises.  (p2's optics branch exists: optics.py.)
``hdbscan`` (no upstream counterpart; the dbscan branch without its eps): an HDBSCAN(min_cluster_size = --hdbscan_min_cluster_size, default feat_dim + 1,
min_samples = feat_dim + 1) fit per cohort on the GPU (hdbscan.py), training clusters re-numbered by sbp, validation / test clusters mapped onto the nearest
training centre, exactly as the dbscan branch does it; writes <cohort>_mcs-<min_cluster_size>.npy.
``--transfer knn`` (dbscan, hdbscan, snn and spectral; no upstream counterpart): only the training cohort is fitted and re-numbered by sbp; every validation / test
encounter takes the label most frequent among its --transfer_k (default feat_dim + 1) nearest training encounters, noise being a label like any other
(knn.knn_transfer_labels: the vote of KNeighborsClassifier).  That works whatever the cohorts' own cluster counts would have been and labels a non-convex
cluster by its members, not its centre.  Writes <cohort>_eps-<opt_eps>_knn.npy / <cohort>_mcs-<min_cluster_size>_knn.npy with ``cluster_id`` and
``cluster_vote``, the winning label's share of the votes (1 for the training cohort).  The default, ``--transfer centre``, is the behaviour above.
``snn`` (no upstream counterpart; the dbscan branch with shared neighbours in place of the euclidean radius): an SNN(n_neighbors = --snn_k, default feat_dim + 1,
eps = --snn_eps shared neighbours, default round(k / 2), min_samples = --snn_min_samples, default k // 4) fit per cohort on the GPU (snn.py), aligned and
transferred exactly as the dbscan branch does it, --transfer knn included; writes <cohort>_snn-k<k>-eps<eps>-ms<min_samples>[_knn].npy.  The two defaults
are starting points, not measured on the real latents.
``spectral`` (no upstream counterpart; a partition into exactly --num_clusters groups that need not be convex): a SpectralClustering(--num_clusters,
n_neighbors = --spectral_k, default 10, assign_labels = --spectral_assign) fit per cohort on the GPU (spectral.py), aligned and transferred exactly as the
dbscan branch does it, --transfer knn included (the method has no predict of its own); writes <cohort>_spectral-k<k>-K<K>[_knn].npy.
``consensus`` (p4:241-287): reads the raw consensus labels of out_feat/raw_consensus_result/<cohort>_consensus.csv (column k<num_clusters>, 0- or 1-based),
re-numbers the training clusters by sbp (generate_align_map) and applies that map to the training and the validation cohort (upstream leaves the test cohort
out); writes <cohort>_<k>.npy.  Upstream's csv files were "generated outside"; a missing one is first computed here by consensus clustering of that cohort's
latents on the GPU (consensus.py) and written.
``ward`` (no upstream counterpart; the kmeans branch with a tree in place of the fits): the Ward tree of the training latents on the GPU (ward.py) cut at
--num_clusters, the clusters re-numbered by sbp, the centres re-ordered with the map; the training cohort keeps its tree labels, validation and test get the
nearest training centre; writes <cohort>_<k>.npy.
``gmm`` (no upstream counterpart; the kmeans branch with a mixture in place of the centres): a Gaussian mixture of --num_clusters components (--gmm_covariance_type, default
diag) fitted to the training latents on the GPU (gmm.py; gmm_full.py for full and tied), the components re-numbered by sbp -- weights, means and covariances permuted with the map -- and every cohort
labelled by ``predict`` of that one model; writes <cohort>_<k>.npy with ``cluster_id`` and ``cluster_prob``, the (N, K) f32 responsibilities.
``fcm`` (no upstream counterpart; the kmeans branch with fuzzy c-means in place of k-means, fcm.py): one fit of the training latents with --num_clusters
centres and the fuzzifier --fcm_m (default 2; a fit whose centres coincide warns: choose a smaller one), the centres re-numbered by sbp and every cohort
labelled by ``predict`` of that one model; writes <cohort>_<k>.npy with ``cluster_id``, ``cluster_prob``, the (N, K) f32 memberships, and ``fcm_m``.
``bgmm`` (no upstream counterpart; the gmm branch with a variational Bayesian mixture, bgmm.py): one fit of the training latents with --num_clusters as the
UPPER bound on the components (--bgmm_concentration, --bgmm_prior_type, --gmm_covariance_type diag | spherical); the active components -- those that are
some training encounter's label -- re-numbered by sbp, every cohort labelled by ``predict`` (a row whose best component is inactive in training gets the
best active one); writes <cohort>_bgmm-K<K>.npy with ``cluster_id`` and ``cluster_prob``, one f32 column per active component.
``meanshift`` (no upstream counterpart; the kmeans branch with the modes of the latent density in place of the centres, their number found by the fit): one
mean shift fit of the training latents on the GPU (meanshift.py) at --meanshift_bandwidth, or at estimate_bandwidth(training latents,
--meanshift_quantile); the centres re-numbered by sbp and every cohort labelled by ``predict``, the nearest centre -- with --meanshift_cluster_all 0 an
encounter farther than the bandwidth from it is an orphan, -1; writes <cohort>_meanshift-bw<bandwidth, %.6g>.npy.
``kmedoids`` (no upstream counterpart; the kmeans branch with medoids -- actual training encounters -- in place of the centres): one k-medoids (PAM) fit of
the training latents on the GPU (kmedoids.py) from BUILD with --num_clusters slots, the slots re-numbered by sbp and every cohort labelled by ``predict``, the
nearest medoid; writes <cohort>_<k>.npy with ``cluster_id`` and, for the training cohort, ``medoid_index``: the rows of the medoid encounters in slot order.
``densitypeaks`` (no upstream counterpart; the kmedoids branch with the density peaks -- again training encounters -- as centres): one density-peaks fit of
the training latents on the GPU (density_peaks.py) at --num_clusters (--dp_k overrides it), density --dp_density (cutoff | knn), d_c = --dp_dc or the
--dp_percent rule, --dp_halo 1 marking the halo encounters -1; the slots re-numbered by sbp; the training cohort keeps the fit's labels, the other cohorts
take the nearest centre (``predict``) or, with --transfer knn, the vote among their nearest training encounters; writes <cohort>_<k>[_knn].npy with
``cluster_id`` and, for the training cohort, ``center_index``: the rows of the centre encounters in slot order.
``--embed tsne`` (no upstream counterpart; beside any --cluster_method): one exact t-SNE fit of the training cohort on the GPU (tsne.py: --tsne_perplexity,
--tsne_max_iter); the validation and test cohorts are PLACED on that map by ``transform`` -- every encounter at the p-weighted mean of its nearest training
encounters' positions -- not embedded again; writes <cohort>_tsne.npy with ``encounter_id``, ``hidden`` and ``tsne`` (N, 2) f64.  Without --embed nothing changes.
``--embed_quality_k 5 10 30`` (with --embed tsne): training_tsne_quality.csv beside training_tsne.npy (k, trustworthiness, continuity, neighbors_kept as
%.17g; embedding_quality.py) -- the training cohort only: the placed cohorts are no fit, and a rank of queries against an index is not built.
``--outlier lof`` (no upstream counterpart; beside any --cluster_method): the local outlier factor (lof.py: sklearn's LocalOutlierFactor) at every k of
--outlier_k (default 20).  The training cohort is FITTED once, one neighbour join for all k; the validation and test cohorts are SCORED against it as new
encounters (sklearn's novelty ``score_samples``), one query join per cohort.  Writes <cohort>_lof.npy with ``encounter_id``, ``ks``, ``lof`` (N, nk) f64 --
the positive factor, about 1 inside a neighbourhood -- and ``outlier`` (N, nk) bool: beyond the TRAINING fit's offset per k (--outlier_contamination:
'auto', the default, is a factor of 1.5; a float in (0, 0.5] is that share of the training cohort).  Without --outlier nothing changes.
``--validity dbcv`` (no upstream counterpart; beside any --cluster_method): the labels written for each cohort are scored against that cohort's own
latents by DBCV (dbcv.py: Density-Based Clustering Validation, one number in [-1, 1] with a place for noise).  Writes <cohort>_dbcv.csv (labelling -- the
label file's name --, n_clusters, n_noise, n_singletons, dbcv; NaN below two clusters) and <cohort>_dbcv_clusters.csv (labelling, cluster, size,
sparseness, separation, nearest_cluster, validity), %.17g, left alone unless overwrite.  Without --validity nothing changes.
``--agreement INDEX [INDEX ...]`` (ari ami nmi rand fmi vmeasure; no upstream counterpart; beside any --cluster_method): for each cohort, once its label
file is written, every <metric>_<m>_aligned/<cohort>_*.npy (--agreement_scope method: this method's directory only) that holds a ``cluster_id`` and the
cohort's own ``encounter_id`` array is compared with every other (agreement.py), named <method>/<file stem>.  Writes <cohort>_agreement.csv: one row per
unordered pair -- labelling_a, labelling_b, n, clusters_a, clusters_b, then the indices, %.17g --, left alone unless overwrite.  --agreement_noise class
(the default: -1 is a class, as in sklearn) or drop.  Labellings of DIFFERENT cohorts are not compared.  Without --agreement nothing changes.
"""
import argparse
import os
import os.path as osp

import numpy as np
import pandas as pd

from ._cluster_cli import (AGREEMENT_COLUMNS, DBCV_CLUSTER_COLUMNS, DBCV_COLUMNS, METHODS, add_agreement_arguments, agreement_summary, cohort_labellings,
                           contamination_arg, dbcv_summary, noise_summary, spell)
from .dbscan import DBSCAN
from .density_peaks import DensityPeaks
from .fcm import FuzzyCMeans
from .bgmm import BayesianGaussianMixture
from .gmm import GaussianMixture
from .gmm_full import FullGaussianMixture
from .hdbscan import HDBSCAN
from .info import COHORTS
from .kmeans import KMeans
from .kmedoids import KMedoids
from .meanshift import MeanShift, estimate_bandwidth
from .knn import knn_transfer_labels
from .snn import SNN
from .spectral import SpectralClustering
from .tsne import TSNE
from .utils import logger, print_dict_byline
from .ward import Ward

np.random.seed(123)        # p4_clustering_final.py:24


def get_arguments(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--cluster_method', default='kmeans', choices=METHODS)
    p.add_argument('--num_clusters', type=int, default=4, help='The number of cluster centers')
    p.add_argument('--gmm_covariance_type', default='diag', choices=['diag', 'spherical', 'full', 'tied'],
                   help='(extra) covariances of --cluster_method gmm; full and tied run gmm_full.py (bgmm: diag or spherical)')
    p.add_argument('--fcm_m', type=float, default=2.0,
                   help='(extra) the fuzzifier of --cluster_method fcm, > 1; default 2 -- a fit that warns of coincident centres wants a smaller one, e.g. 1.2')
    p.add_argument('--bgmm_concentration', type=float, default=None,
                   help='(extra) weight concentration prior of --cluster_method bgmm (default: 1 / num_clusters)')
    p.add_argument('--bgmm_prior_type', default='dirichlet_process', choices=['dirichlet_process', 'dirichlet_distribution'],
                   help='(extra) the weight prior of --cluster_method bgmm')
    p.add_argument('--restore_metric', default=['ae_mse', 'loss', 'delta'])
    p.add_argument('--opt_eps', type=float, default=1.9)
    p.add_argument('--hdbscan_min_cluster_size', type=int, default=None, help='(extra) min_cluster_size of --cluster_method hdbscan; default feat_dim + 1')
    p.add_argument('--snn_k', type=int, default=None, help='(extra) neighbours per point of --cluster_method snn; default feat_dim + 1')
    p.add_argument('--snn_eps', type=int, default=None,
                   help='(extra) shared-neighbour threshold of --cluster_method snn, an integer in [1, k]; default round(k / 2) -- a starting point, not '
                        "measured on the real latents: read it from p2's plot/snn_similarity_hist.csv")
    p.add_argument('--snn_min_samples', type=int, default=None,
                   help='(extra) strong links that make a core point of --cluster_method snn (0: Jarvis-Patrick); default k // 4 -- a starting point, not '
                        'measured on the real latents')
    p.add_argument('--spectral_k', type=int, default=10, help="(extra) neighbours per point of --cluster_method spectral; default 10, sklearn's")
    p.add_argument('--spectral_assign', default='kmeans', choices=['kmeans', 'cluster_qr'], help='(extra) how --cluster_method spectral labels the embedding')
    p.add_argument('--meanshift_bandwidth', type=float, default=None, help='(extra) bandwidth of --cluster_method meanshift')
    p.add_argument('--meanshift_quantile', type=float, default=None,
                   help='(extra) without --meanshift_bandwidth: estimate_bandwidth(training latents, quantile); default 0.3, sklearn\'s')
    p.add_argument('--meanshift_bin_seeding', action='store_true', help="(extra) seed --cluster_method meanshift from sklearn's bins, not from every point")
    p.add_argument('--meanshift_cluster_all', type=int, default=1, choices=[1, 0],
                   help='(extra) 0: an encounter farther than the bandwidth from its nearest centre is an orphan (-1), in every cohort')
    p.add_argument('--dp_density', default='cutoff', choices=['cutoff', 'knn'], help='(extra) density of --cluster_method densitypeaks')
    p.add_argument('--dp_percent', type=float, default=2.0,
                   help='(extra) --cluster_method densitypeaks: d_c is the radius at which a point has on average this percentage of the cohort as neighbours')
    p.add_argument('--dp_dc', type=float, default=None, help='(extra) d_c of --cluster_method densitypeaks; overrides --dp_percent')
    p.add_argument('--dp_k', type=int, default=None, help='(extra) clusters of --cluster_method densitypeaks; default --num_clusters')
    p.add_argument('--dp_halo', type=int, default=0, choices=[0, 1], help='(extra) 1: halo encounters of --cluster_method densitypeaks are labelled -1 (cutoff only)')
    p.add_argument('--transfer', default='centre', choices=['centre', 'knn'],
                   help="(extra) how --cluster_method dbscan / hdbscan / snn / spectral label the validation and test cohorts: 'centre' fits each cohort and maps its clusters onto "
                        "the nearest training centre (upstream); 'knn' fits the training cohort only and votes among the nearest training encounters")
    p.add_argument('--transfer_k', type=int, default=None, help='(extra) neighbours of --transfer knn; default feat_dim + 1')
    p.add_argument('--dl_cluster_label_type', default='pred', choices=['label', 'pred'])
    p.add_argument('--embed', default=None, choices=['tsne'],
                   help='(extra) also write a two-dimensional map of every cohort (<cohort>_tsne.npy): one fit of the training cohort, the others placed on it')
    p.add_argument('--tsne_perplexity', type=float, default=30.0, help="(extra) perplexity of --embed tsne; default 30, sklearn's")
    p.add_argument('--tsne_max_iter', type=int, default=1000, help="(extra) iterations of --embed tsne; default 1000, sklearn's (250 of them exaggerated)")
    p.add_argument('--embed_quality_k', type=int, nargs='+', default=None,
                   help='(extra) with --embed tsne: also write trustworthiness, continuity and the share of neighbours kept of the training map at these '
                        'neighbourhood sizes (training_tsne_quality.csv), e.g. 5 10 30')
    p.add_argument('--outlier', default=None, choices=['lof'],
                   help='(extra) also write the local outlier factor of every cohort (<cohort>_lof.npy): one fit of the training cohort, the others scored against it')
    p.add_argument('--outlier_k', type=int, nargs='+', default=[20], help="(extra) neighbourhood sizes of --outlier lof, one join for all; default 20, sklearn's")
    p.add_argument('--validity', default=None, choices=['dbcv'],
                   help='(extra) also score the labels written for each cohort by DBCV on that cohort\'s latents (<cohort>_dbcv.csv, <cohort>_dbcv_clusters.csv)')
    p.add_argument('--outlier_contamination', type=contamination_arg, default='auto',
                   help="(extra) --outlier lof: 'auto' (an encounter is an outlier beyond a factor of 1.5) or the share of outliers in the training cohort, a "
                        'float in (0, 0.5]')
    add_agreement_arguments(p, "each cohort's label files on disk (<cohort>_agreement.csv)")
    return p.parse_args(argv)


class Cluster(object):
    KEEP = ['encounter_id', 'hidden', 'ob', 'padding_mask']

    def __init__(self, args):
        self.args = args
        self.exp_path = os.path.join(os.getcwd(), 'Results', 'Clustering')

    def load_data(self):
        keep = self.KEEP + (['cluster_pred', 'cluster_label'] if self.args.cluster_method == 'dl' else [])
        cohorts = []
        for cohort in COHORTS:
            full = np.load(osp.join(self.feat_path, '{}.npy'.format(cohort)), allow_pickle=True).item()
            cohorts.append({k: full[k] for k in keep})
            logger.info('Cohort: {}, Sample: {}'.format(cohort, len(full['encounter_id'])))
        self.train_data, self.valid_data, self.test_data = cohorts
        self.feat_dim = self.train_data['hidden'].shape[-1]

    def generate_align_map(self, org_label, ob, padding, feat=None):
        """{old id -> new id} with new ids ordered by descending per-cluster mean of channel 0 (sbp)."""
        pad0 = padding[:, 0, :]
        per_enc = np.sum(ob[:, 0, :] * pad0, axis=1) / np.sum(pad0, axis=1)
        n_clusters = len(set(org_label)) - (1 if -1 in org_label else 0)
        members = [np.where(org_label == i) for i in range(n_clusters)]
        order = np.argsort([np.average(per_enc[m]) for m in members])[::-1]
        align_map = {int(prev): cur for cur, prev in enumerate(order)}
        align_map = {k: align_map[k] for k in sorted(align_map)}
        logger.info('Align_map: {}'.format(align_map))
        for old, new in align_map.items():
            org_label[members[old]] = new
        centers = [np.mean(feat[org_label == i], axis=0) for i in range(n_clusters)] if feat is not None else []
        return align_map, org_label, centers

    def align_labels_with_center(self, org_feat, org_label, aligned_feat_centers):
        """p4:113-139: each cluster of ``org_label`` takes the id of the nearest of ``aligned_feat_centers`` (the training clusters' centres); two clusters
        mapped onto one centre raise ValueError.  Noise (-1) stays -1."""
        n_clusters = len(set(org_label)) - (1 if -1 in org_label else 0)
        org_centers = np.asarray([np.mean(org_feat[org_label == i], axis=0) for i in range(n_clusters)], dtype=np.float64)
        ref = np.asarray(aligned_feat_centers, dtype=np.float64)
        d = np.sqrt(np.maximum((org_centers ** 2).sum(1)[:, None] + (ref ** 2).sum(1)[None, :] - 2.0 * org_centers @ ref.T, 0.0))
        min_dist_idx = np.argmin(d, axis=1)
        if len(set(min_dist_idx)) != n_clusters:
            logger.info(min_dist_idx)
            raise ValueError('Different org_feat_centers map to a same train_feat_center')
        align_map = {org_id: new_id for org_id, new_id in enumerate(min_dist_idx)}
        logger.info('Align_map: {}'.format(align_map))
        members = [np.where(org_label == i) for i in range(n_clusters)]
        for org_id, new_id in align_map.items():
            org_label[members[org_id]] = new_id
        return org_label

    def _knn_labels(self, f_train, train_ref, feat):
        """--transfer knn: ``(cluster_id, cluster_vote)`` of a validation / test cohort from the training latents and their aligned labels -- ``train_ref``
        as the training cohort left it in this run, else read back from the training file ``f_train`` of an earlier one."""
        if train_ref is None:
            if not osp.exists(f_train):
                raise ValueError('--transfer knn: the training cohort has no labels to transfer (no cluster was found, or {} is missing)'.format(f_train))
            done = np.load(f_train, allow_pickle=True).item()
            train_ref = (done['hidden'], done['cluster_id'])
        k = self.args.transfer_k if getattr(self.args, 'transfer_k', None) is not None else self.feat_dim + 1
        logger.info('kNN label transfer from {} training encounters, k: {}'.format(len(train_ref[1]), k))
        label, vote = knn_transfer_labels(train_ref[0], np.asarray(train_ref[1]).astype(np.int64), feat, k)
        return label.astype(np.asarray(train_ref[1]).dtype), vote

    @property
    def knn(self):
        """--transfer knn (an args object from before the flag: the default, centre)."""
        return getattr(self.args, 'transfer', 'centre') == 'knn'

    def _reorder(self, model, raw_label):
        """Re-numbers the clusters of a model of the training cohort by sbp: ``generate_align_map`` of its 0-based training labels, then the model's
        slots permuted with the map -- by ``model.reorder``, or for KMeans and Ward, which have none, by permuting ``cluster_centers_`` in place -- so
        that ``predict`` answers in the new ids.  Returns the aligned training labels."""
        align_map, aligned, _ = self.generate_align_map(raw_label, self.train_data['ob'], self.train_data['padding_mask'])
        order = np.empty(len(align_map), dtype=np.int64)
        for old, new in align_map.items():
            order[new] = old
        if hasattr(model, 'reorder'):
            model.reorder(order)
        else:
            model.cluster_centers_[:] = model.cluster_centers_[order]
        return aligned

    def _write_cohorts(self, cohorts, overwrite, name, fill):
        """Writes ``name.format(cohort)`` for every cohort that has no such file yet (or all, with ``overwrite``): ``fill(cohort, data)`` puts
        ``cluster_id`` and any extras into the cohort's dict, which is saved without ``ob`` and ``padding_mask``.  A ``fill`` that returns False has
        nothing to write for its cohort."""
        for cohort, data in cohorts:
            f = osp.join(self.out_path, name.format(cohort))
            if osp.exists(f) and not overwrite:
                logger.info('Not Save for {}.'.format(f))
                continue
            if fill(cohort, data) is False:
                continue
            del data['ob'], data['padding_mask']
            np.save(f, data)
            logger.info('Cohort clustering: {} is done. Save to {}'.format(cohort, f))
            self._validity_dbcv(cohort, data, f, overwrite)

    def _validity_dbcv(self, cohort, data, label_file, overwrite):
        """--validity dbcv: the DBCV of the ``cluster_id`` just written to ``label_file`` on the cohort's own latents.  Writes <cohort>_dbcv.csv and
        <cohort>_dbcv_clusters.csv (``dbcv_summary``'s two tables, %.17g), left alone where both exist unless ``overwrite``."""
        if getattr(self.args, 'validity', None) != 'dbcv':          # (an args object from before the flag: no scores)
            return
        files = [osp.join(self.out_path, '{}_{}.csv'.format(cohort, name)) for name in ('dbcv', 'dbcv_clusters')]
        if all(osp.exists(f) for f in files) and not overwrite:
            logger.info('Not Save for {}.'.format(files[0]))
            return
        rows, cluster_rows = dbcv_summary(np.asarray(data['hidden'], dtype=np.float32), {osp.basename(label_file): np.asarray(data['cluster_id'])})
        pd.DataFrame(rows, columns=DBCV_COLUMNS).to_csv(files[0], index=False, float_format='%.17g')
        pd.DataFrame(cluster_rows, columns=DBCV_CLUSTER_COLUMNS).to_csv(files[1], index=False, float_format='%.17g')
        logger.info('Cohort DBCV: {} is done. Save to {}'.format(cohort, files[0]))

    def _agreement(self, cohorts, overwrite):
        """--agreement: per cohort, the label files on disk (``cohort_labellings``) compared with each other.  Writes <cohort>_agreement.csv
        (``agreement_summary``'s long table, %.17g), left alone where it exists unless ``overwrite``; fewer than two labellings: logged, nothing written."""
        indices = list(dict.fromkeys(self.args.agreement))
        methods = METHODS if getattr(self.args, 'agreement_scope', 'all') == 'all' else [self.args.cluster_method]
        metric = osp.basename(self.feat_path)
        for cohort, data in cohorts:
            f = osp.join(self.out_path, '{}_agreement.csv'.format(cohort))
            if osp.exists(f) and not overwrite:
                logger.info('Not Save for {}.'.format(f))
                continue
            labellings = cohort_labellings(osp.dirname(self.out_path), metric, methods, cohort, data['encounter_id'])
            if len(labellings) < 2:
                logger.info('No agreement for the {} cohort: {} labelling on disk, two are needed.'.format(cohort, len(labellings)))
                continue
            rows, _ = agreement_summary(labellings, indices, getattr(self.args, 'agreement_noise', 'class'))
            pd.DataFrame(rows, columns=AGREEMENT_COLUMNS + indices).to_csv(f, index=False, float_format='%.17g')
            logger.info('Cohort agreement: {} is done. Save to {}'.format(cohort, f))

    def _density_branch(self, cohorts, overwrite, name, title, fit):
        """The dbscan, hdbscan, snn and spectral branches: ``fit(feat) -> (raw labels, core points or None)`` per cohort, training clusters re-numbered by
        sbp, validation / test clusters mapped onto the nearest training centre -- or, with --transfer knn, only the training cohort fitted and the others
        voted (``_knn_labels``).  ``name``: the file name with the cohort left open, without '_knn' and '.npy'; ``title``: the method's name in the log."""
        name += ('_knn' if self.knn else '') + '.npy'
        train_feat_centers = train_ref = None

        def fill(cohort, data):
            nonlocal train_feat_centers, train_ref
            feat = data['hidden']
            n_core = None
            if self.knn and cohort != 'training':
                aligned_label, data['cluster_vote'] = self._knn_labels(osp.join(self.out_path, name.format('training')), train_ref, feat)
            else:
                logger.info('NEW {} model for {}'.format(title, cohort))
                raw_label, n_core = fit(feat)
                if cohort == 'training':
                    _, aligned_label, train_feat_centers = self.generate_align_map(raw_label, data['ob'], data['padding_mask'], feat)
                else:
                    aligned_label = self.align_labels_with_center(feat, raw_label, train_feat_centers)
                if self.knn:
                    train_ref = (feat, aligned_label)
                    data['cluster_vote'] = np.ones(len(aligned_label), dtype=np.float32)
            data['cluster_id'] = aligned_label
            return noise_summary(feat, aligned_label, n_core)[0] > 0          # (no cluster: upstream writes nothing for this cohort either)
        self._write_cohorts(cohorts, overwrite, name, fill)

    def _kmeans(self, cohorts, overwrite):
        k = self.args.num_clusters
        logger.info('==> Generate the k-means results with opt-k: {}'.format(k))
        model = KMeans(n_clusters=k, init='k-means++', n_init=20).fit(self.train_data['hidden'])
        self._reorder(model, model.predict(self.train_data['hidden']))
        self._write_cohorts(cohorts, overwrite, '{{}}_{}.npy'.format(k), lambda cohort, data: data.update(cluster_id=model.predict(data['hidden'])))

    def _dl(self, cohorts, overwrite):
        for cohort, data in cohorts:          # (not _write_cohorts: the file name comes from the cohort's own soft assignment)
            prob = data['cluster_label'] if self.args.dl_cluster_label_type == 'label' else data['cluster_pred']
            data['cluster_id'] = np.argmax(prob, 1)
            del data['cluster_pred'], data['cluster_label']
            f = osp.join(self.out_path, '{}_{}.npy'.format(cohort, prob.shape[1]))
            if osp.exists(f) and not overwrite:
                logger.info('Not Save for {}.'.format(f))
                continue
            np.save(f, data)
            logger.info('Cohort clustering: {} is done. Save to {}'.format(cohort, f))
            self._validity_dbcv(cohort, data, f, overwrite)

    def _dbscan(self, cohorts, overwrite):
        opt_eps = self.args.opt_eps
        logger.info('==> Generate the DBSCAN results with opt-eps: {}'.format(opt_eps))

        def fit(feat):
            db = DBSCAN(opt_eps, feat.shape[-1]).fit(feat)
            return db.labels_, len(db.core_sample_indices_)
        self._density_branch(cohorts, overwrite, '{{}}_eps-{}'.format(opt_eps), 'DBSCAN', fit)

    def _hdbscan(self, cohorts, overwrite):
        min_samples = self.feat_dim + 1
        mcs = self.args.hdbscan_min_cluster_size if self.args.hdbscan_min_cluster_size is not None else self.feat_dim + 1
        logger.info('==> Generate the HDBSCAN results with min_cluster_size: {}, min_samples: {}'.format(mcs, min_samples))
        self._density_branch(cohorts, overwrite, '{{}}_mcs-{}'.format(mcs), 'HDBSCAN',
                             lambda feat: (HDBSCAN(min_cluster_size=mcs, min_samples=min_samples).fit(feat).labels_, None))

    def _snn(self, cohorts, overwrite):
        """The dbscan branch with shared neighbours in place of the euclidean radius: SNN(--snn_k, --snn_eps, --snn_min_samples) per cohort."""
        k = self.args.snn_k if self.args.snn_k is not None else self.feat_dim + 1
        eps = self.args.snn_eps if self.args.snn_eps is not None else int(round(k * 0.5))
        ms = self.args.snn_min_samples if self.args.snn_min_samples is not None else k // 4
        logger.info('==> Generate the SNN results with k: {}, eps: {}, min_samples: {}'.format(k, eps, ms))

        def fit(feat):
            sn = SNN(k, eps, ms).fit(feat)
            return sn.labels_, len(sn.core_sample_indices_)
        self._density_branch(cohorts, overwrite, '{{}}_snn-k{}-eps{}-ms{}'.format(k, eps, ms), 'SNN', fit)

    def _spectral(self, cohorts, overwrite):
        """The dbscan branch with a spectral partition into --num_clusters groups in place of the density clusters (no noise label, no core points)."""
        K, k, assign = self.args.num_clusters, self.args.spectral_k, self.args.spectral_assign
        logger.info('==> Generate the spectral clustering results with opt-k: {}, neighbours: {}, assign_labels: {}'.format(K, k, assign))
        self._density_branch(cohorts, overwrite, '{{}}_spectral-k{}-K{}'.format(k, K), 'spectral clustering',
                             lambda feat: (SpectralClustering(K, n_neighbors=k, assign_labels=assign).fit(feat).labels_, None))

    def _ward(self, cohorts, overwrite):
        """The kmeans branch with one Ward tree of the training latents in place of the k-means fits: the tree is cut at --num_clusters, generate_align_map
        orders the clusters by sbp and the centres (the means of the members) are re-ordered with the map.  The training cohort keeps its tree labels,
        aligned; validation and test get ``predict``, the nearest aligned training centre.  A training point's tree label need not be its nearest centre
        -- Ward merges greedily and never reassigns a point -- so the training ids are NOT ``predict`` of the training latents, unlike the kmeans branch."""
        k = self.args.num_clusters
        logger.info('==> Generate the Ward results with opt-k: {}'.format(k))
        model = Ward(n_clusters=k).fit(self.train_data['hidden'])
        aligned = self._reorder(model, np.array(model.labels_))
        self._write_cohorts(cohorts, overwrite, '{{}}_{}.npy'.format(k),
                            lambda cohort, data: data.update(cluster_id=aligned if cohort == 'training' else model.predict(data['hidden'])))

    def _gmm(self, cohorts, overwrite):
        """The kmeans branch with a Gaussian mixture in place of the centres: fitted on the training cohort, generate_align_map orders the components by sbp
        and the model's weights, means and covariances are permuted with the map, as the kmeans branch permutes its centres.  Every cohort, training
        included, is labelled by ``predict`` of that model; ``cluster_prob`` holds its responsibilities, so ``cluster_id`` is their argmax."""
        k = self.args.num_clusters
        logger.info('==> Generate the Gaussian mixture results with opt-k: {}'.format(k))
        cov = self.args.gmm_covariance_type
        cls = FullGaussianMixture if cov in ('full', 'tied') else GaussianMixture
        model = cls(n_components=k, n_init=10, covariance_type=cov).fit(self.train_data['hidden'])
        raw = model.predict(self.train_data['hidden']).astype(np.int64)
        if len(set(raw)) != k:
            raise ValueError('the Gaussian mixture left {} of its {} components without a training encounter: choose a smaller --num_clusters'.format(
                k - len(set(raw)), k))
        self._reorder(model, raw)
        self._write_cohorts(cohorts, overwrite, '{{}}_{}.npy'.format(k), lambda cohort, data: data.update(
            cluster_id=model.predict(data['hidden']), cluster_prob=model.predict_proba(data['hidden']).astype(np.float32)))

    def _fcm(self, cohorts, overwrite):
        """The kmeans branch with fuzzy c-means in place of k-means: one fit of the training cohort, generate_align_map orders the centres by sbp as the
        gmm branch orders its components and the model is permuted with the map.  Every cohort, training included, is labelled by ``predict`` of that
        model; ``cluster_prob`` holds its memberships, so ``cluster_id`` is their first maximum, and ``fcm_m`` the fuzzifier they were formed with."""
        k, m = self.args.num_clusters, float(self.args.fcm_m)
        logger.info('==> Generate the fuzzy c-means results with opt-k: {}, m: {:g}'.format(k, m))
        model = FuzzyCMeans(n_clusters=k, m=m, n_init=10).fit(self.train_data['hidden'])
        raw = model.labels_.astype(np.int64)
        if len(set(raw.tolist())) != k:
            raise ValueError('fuzzy c-means left {} of its {} centres without a training encounter: choose a smaller --num_clusters or a smaller '
                             '--fcm_m'.format(k - len(set(raw.tolist())), k))
        self._reorder(model, raw)
        self._write_cohorts(cohorts, overwrite, '{{}}_{}.npy'.format(k), lambda cohort, data: data.update(
            cluster_id=model.predict(data['hidden']), cluster_prob=model.predict_proba(data['hidden']).astype(np.float32), fcm_m=m))

    def _bgmm(self, cohorts, overwrite):
        """The gmm branch with a variational Bayesian mixture of --num_clusters components: one fit of the training cohort, whose prior empties the
        components the latents do not support.  The ACTIVE components -- the labels of at least one training encounter -- are ordered by sbp as the gmm
        branch orders its components; every cohort is labelled by ``predict`` of that model, and a row whose best component is inactive in training
        gets the best active one.  ``cluster_prob`` holds the model's responsibilities of the active components, one column each, in the new order."""
        k = self.args.num_clusters
        cov = self.args.gmm_covariance_type
        logger.info('==> Generate the Bayesian Gaussian mixture results with at most {} components'.format(k))
        model = BayesianGaussianMixture(n_components=k, n_init=10, covariance_type=cov, weight_concentration_prior_type=self.args.bgmm_prior_type,
                                        weight_concentration_prior=self.args.bgmm_concentration).fit(self.train_data['hidden'])
        active = model.active_components_
        raw = np.searchsorted(active, model.labels_).astype(np.int64)
        align_map, _, _ = self.generate_align_map(raw, self.train_data['ob'], self.train_data['padding_mask'])
        columns = np.empty(len(active), dtype=np.int64)
        for old, new in align_map.items():
            columns[new] = active[old]
        logger.info('Active components: {} of {} ({}); a row whose best component is inactive in training gets the best active one.'.format(
            len(active), k, columns.tolist()))

        def fill(cohort, data):
            prob = model.predict_proba(data['hidden'])[:, columns]
            data.update(cluster_id=np.argmax(prob, axis=1).astype(np.int64), cluster_prob=prob.astype(np.float32))
        self._write_cohorts(cohorts, overwrite, '{{}}_bgmm-K{}.npy'.format(k), fill)

    def _meanshift(self, cohorts, overwrite):
        """The kmeans branch with mean shift in place of k-means: one fit of the training cohort at the given or the estimated bandwidth finds the centres and
        their number, generate_align_map orders them by sbp and the centres are permuted with the map.  Every cohort, training included, is labelled by
        ``predict`` of that model (the training cohort's ``labels_`` are exactly that), with the orphan rule when --meanshift_cluster_all is 0."""
        h = self.args.meanshift_bandwidth
        if h is None:
            q = self.args.meanshift_quantile if self.args.meanshift_quantile is not None else 0.3
            h = estimate_bandwidth(self.train_data['hidden'], q)
        cluster_all = bool(self.args.meanshift_cluster_all)
        logger.info('==> Generate the mean shift results with bandwidth: {:.6g}, cluster_all: {}'.format(h, cluster_all))
        model = MeanShift(bandwidth=h, bin_seeding=self.args.meanshift_bin_seeding, cluster_all=cluster_all).fit(self.train_data['hidden'])
        k = len(model.cluster_centers_)
        raw = np.array(model.labels_)
        if set(raw.tolist()) - {-1} != set(range(k)):
            raise ValueError('mean shift left {} of its {} centres without a training encounter: choose another bandwidth'.format(
                k - len(set(raw.tolist()) - {-1}), k))
        logger.info('Estimated number of clusters: {}, orphans: {}'.format(k, int(np.sum(raw == -1))))
        self._reorder(model, raw)
        self._write_cohorts(cohorts, overwrite, '{{}}_meanshift-bw{:.6g}.npy'.format(h),
                            lambda cohort, data: data.update(cluster_id=model.predict(data['hidden'], orphans=not cluster_all)))

    def _kmedoids(self, cohorts, overwrite):
        """The kmeans branch with k-medoids (PAM) in place of k-means: one fit of the training cohort from BUILD, generate_align_map orders the slots by sbp and
        the medoids are permuted with the map.  Every cohort, training included, is labelled by ``predict`` of that model, the nearest medoid (the training
        cohort's ``labels_`` are exactly that); the training cohort's file also holds ``medoid_index``, the rows of the medoid encounters in slot order."""
        k = self.args.num_clusters
        logger.info('==> Generate the k-medoids results with opt-k: {}'.format(k))
        model = KMedoids(n_clusters=k).fit(self.train_data['hidden'])
        self._reorder(model, np.array(model.labels_))

        def fill(cohort, data):
            data['cluster_id'] = model.predict(data['hidden'])
            if cohort == 'training':
                data['medoid_index'] = model.medoid_indices_.copy()
        self._write_cohorts(cohorts, overwrite, '{{}}_{}.npy'.format(k), fill)

    def _densitypeaks(self, cohorts, overwrite):
        """The kmedoids branch with density peaks in place of PAM: one fit of the training cohort, generate_align_map orders the slots by sbp (from the
        labels without the halo) and the model is permuted with the map.  The training cohort keeps the fit's ``labels_``; the other cohorts take
        ``predict``, the nearest centre, or with --transfer knn the vote among the nearest training encounters.  The training cohort's file also holds
        ``center_index``, the rows of the centre encounters in slot order."""
        a = self.args
        k = a.dp_k if getattr(a, 'dp_k', None) is not None else a.num_clusters
        logger.info('==> Generate the density-peaks results with k: {}, density: {}'.format(k, a.dp_density))
        model = DensityPeaks(n_clusters=k, density=a.dp_density, dc='auto' if a.dp_dc is None else a.dp_dc, percent=a.dp_percent,
                             halo=bool(a.dp_halo)).fit(self.train_data['hidden'])
        self._reorder(model, np.array(model.core_labels_))
        train_ref = (np.asarray(self.train_data['hidden']), np.array(model.labels_))

        def fill(cohort, data):
            if cohort == 'training':
                data['cluster_id'] = model.labels_.copy()
                data['center_index'] = model.center_indices_.copy()
                if self.knn:
                    data['cluster_vote'] = np.ones(len(model.labels_), dtype=np.float32)
            elif self.knn:
                data['cluster_id'], data['cluster_vote'] = self._knn_labels(None, train_ref, data['hidden'])
            else:
                data['cluster_id'] = model.predict(data['hidden'])
        self._write_cohorts(cohorts, overwrite, '{{}}_{}{}.npy'.format(k, '_knn' if self.knn else ''), fill)

    def _embed_tsne(self, cohorts, overwrite):
        """--embed tsne: one exact t-SNE fit of the training cohort (tsne.py: init 'pca', --tsne_perplexity, --tsne_max_iter); the validation and test
        cohorts are PLACED on that map by ``transform`` (every encounter at the p-weighted mean of its nearest training encounters' positions), not
        embedded again.  Writes <cohort>_tsne.npy: ``encounter_id``, ``hidden`` and ``tsne`` (N, 2) f64, in the cohort's row order.  With --embed_quality_k
        also training_tsne_quality.csv (k, trustworthiness, continuity, neighbors_kept) of the fitted map -- the training cohort only."""
        files = [osp.join(self.out_path, '{}_tsne.npy'.format(cohort)) for cohort, _ in cohorts]
        quality_k = getattr(self.args, 'embed_quality_k', None)          # (an args object from before the flag: no table)
        quality_csv = osp.join(self.out_path, 'training_tsne_quality.csv')
        if all(osp.exists(f) for f in files + ([quality_csv] if quality_k else [])) and not overwrite:
            logger.info('Not Save for {}.'.format(files[0]))
            return
        logger.info('==> Generate the t-SNE map with perplexity: {}'.format(self.args.tsne_perplexity))
        model = TSNE(perplexity=self.args.tsne_perplexity, max_iter=self.args.tsne_max_iter, init='pca').fit(self.train_data['hidden'])
        logger.info('t-SNE n_iter: {}, kl: {:.6f}'.format(model.n_iter_, model.kl_divergence_))
        if quality_k and (overwrite or not osp.exists(quality_csv)):
            quality = model.quality([int(k) for k in quality_k])
            pd.DataFrame([(k,) + quality[k] for k in sorted(quality)], columns=['k', 'trustworthiness', 'continuity', 'neighbors_kept']).to_csv(
                quality_csv, index=False, float_format='%.17g')
            logger.info('Map quality: training is done. Save to {}'.format(quality_csv))
        for (cohort, data), f in zip(cohorts, files):
            if osp.exists(f) and not overwrite:
                logger.info('Not Save for {}.'.format(f))
                continue
            tsne = model.embedding_.copy() if cohort == 'training' else model.transform(data['hidden'])
            np.save(f, {'encounter_id': data['encounter_id'], 'hidden': data['hidden'], 'tsne': tsne})
            logger.info('Cohort map: {} is done. Save to {}'.format(cohort, f))

    def _outlier_lof(self, cohorts, overwrite):
        """--outlier lof: one fit of the training cohort at every k of --outlier_k (``lof.LofSweep``: one neighbour join); the validation and test cohorts
        are scored against it as new encounters, one query join each.  Writes <cohort>_lof.npy: ``encounter_id``, ``ks``, ``lof`` (N, nk) f64 = the
        positive factor and ``outlier`` (N, nk) bool = beyond the training fit's offset, in the cohort's row order."""
        files = [osp.join(self.out_path, '{}_lof.npy'.format(cohort)) for cohort, _ in cohorts]
        if all(osp.exists(f) for f in files) and not overwrite:
            logger.info('Not Save for {}.'.format(files[0]))
            return
        from .lof import LofSweep          # (here, not at module scope: a run without --outlier loads nothing of it)
        ks = sorted(set(int(k) for k in self.args.outlier_k))
        logger.info('==> Generate the local outlier factors with k: {}'.format(ks))
        model = LofSweep(np.asarray(self.train_data['hidden'], dtype=np.float32), ks, contamination=self.args.outlier_contamination)
        for (cohort, data), f in zip(cohorts, files):
            if osp.exists(f) and not overwrite:
                logger.info('Not Save for {}.'.format(f))
                continue
            nof = model.nof if cohort == 'training' else model.score_samples(np.asarray(data['hidden'], dtype=np.float32))
            np.save(f, {'encounter_id': data['encounter_id'], 'ks': np.asarray(ks, dtype=np.int64), 'lof': -nof, 'outlier': nof < model.offsets[None, :]})
            logger.info('Cohort outlier factors: {} is done. Save to {}'.format(cohort, f))

    def _raw_consensus(self, cohort, data):
        """The raw consensus labels of a cohort for k = num_clusters, 0-based as generate_align_map wants them (p4:247-253): column k<num_clusters> of
        raw_consensus_result/<cohort>_consensus.csv, computed and written first where the file is missing."""
        col = 'k{}'.format(self.args.num_clusters)
        raw_dir = osp.join(self.exp_path, 'out_feat', 'raw_consensus_result')
        f = osp.join(raw_dir, '{}_consensus.csv'.format(cohort))
        if not osp.exists(f):
            from .consensus import ConsensusKMeans          # (the GPU is touched only when a file has to be made)
            logger.info('NEW consensus clustering for {}: {}'.format(cohort, f))
            os.makedirs(raw_dir, exist_ok=True)
            cc = ConsensusKMeans([self.args.num_clusters]).fit(np.asarray(data['hidden'], dtype=np.float32))
            pd.DataFrame({col: cc.labels_[self.args.num_clusters]}).to_csv(f, index=False)
        raw_label = pd.read_csv(f)[col].values
        if not any(raw_label == 0):
            raw_label = raw_label - 1          # adjust label starting from 0, to be comparable to generate_align_map
        return raw_label

    @staticmethod
    def renumber_consensus(raw_label, align_map):
        """p4:273-279: the 0-based raw labels through ``align_map`` {old id: new id}.  Mapped ids are parked as negatives (and new id 0 under a spare tag)
        so that an id already mapped is not mapped again."""
        raw_label = np.array(raw_label)
        tag = max(align_map.keys()) + 10
        for org_id, new_id in align_map.items():
            if new_id == 0:          # label the 0 as None
                raw_label[raw_label == org_id] = tag
            raw_label[raw_label == org_id] = -new_id
        raw_label[raw_label == tag] = 0
        return abs(raw_label)

    def _consensus(self, cohorts, overwrite):
        opt_k = self.args.num_clusters
        logger.info('==> Generate the consensus clustering results with opt-k: {}'.format(opt_k))
        train_raw_label = self._raw_consensus('training', self.train_data)
        align_map, _, _ = self.generate_align_map(train_raw_label, self.train_data['ob'], self.train_data['padding_mask'])
        # the training and the validation cohort only: upstream leaves the test cohort out
        self._write_cohorts(cohorts[:2], overwrite, '{{}}_{}.npy'.format(opt_k),
                            lambda cohort, data: data.update(cluster_id=self.renumber_consensus(self._raw_consensus(cohort, data), align_map)))

    # --cluster_method -> its branch, called with (cohorts, overwrite).  A method of METHODS without an entry ('optics') raises in pred.
    BRANCHES = {'kmeans': _kmeans, 'dl': _dl, 'dbscan': _dbscan, 'consensus': _consensus, 'hdbscan': _hdbscan, 'snn': _snn, 'spectral': _spectral,
                'ward': _ward, 'gmm': _gmm, 'fcm': _fcm, 'meanshift': _meanshift, 'kmedoids': _kmedoids, 'densitypeaks': _densitypeaks, 'bgmm': _bgmm}

    def pred(self, **kwargs):
        overwrite = kwargs.get('overwrite', False)
        transfer = getattr(self.args, 'transfer', 'centre')          # (an args object from before the flag: the default)
        if transfer != 'centre' and self.args.cluster_method not in ('dbscan', 'hdbscan', 'snn', 'spectral', 'densitypeaks'):
            raise ValueError("--transfer {} applies to --cluster_method dbscan and hdbscan only (and to snn, spectral and densitypeaks): '{}' labels every cohort with its training model "
                             "already".format(transfer, self.args.cluster_method))
        for metric in self.args.restore_metric:
            self.feat_path = osp.join(self.exp_path, 'out_feat', metric)
            self.out_path = osp.join(self.exp_path, 'out_feat', '{}_{}'.format(metric, self.args.cluster_method)) + '_aligned'
            os.makedirs(self.out_path, exist_ok=True)
            self.load_data()
            cohorts = list(zip(COHORTS, [self.train_data, self.valid_data, self.test_data]))
            if getattr(self.args, 'embed', None) == 'tsne':          # (an args object from before the flag: no map)
                self._embed_tsne(cohorts, overwrite)
            if getattr(self.args, 'outlier', None) == 'lof':          # (an args object from before the flag: no scores)
                self._outlier_lof(cohorts, overwrite)
            branch = self.BRANCHES.get(self.args.cluster_method)
            if branch is None:
                raise NotImplementedError("only {} are on the accelerated path: upstream's 'optics' branch of p4 is an empty `pass` (p2 has the OPTICS fit)".format(
                    spell(repr(m) for m in self.BRANCHES)))
            branch(self, cohorts, overwrite)
            if getattr(self.args, 'agreement', None):          # (an args object from before the flag: no tables)
                self._agreement(cohorts, overwrite)


def main(args):
    Cluster(args).pred()


if __name__ == '__main__':
    _args = get_arguments()
    print_dict_byline(vars(_args))
    main(_args)
