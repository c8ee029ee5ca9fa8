"""What p2 and p4 share (_cluster_cli.py): the method tuple against both programs' dispatch tables and parsers, and the host logic of the
--internal_metrics of one labelling, which used to stand once per p2 branch."""
import argparse

import numpy as np
import pytest

from deep_interpolation_clustering_amd import _cluster_cli as cli

NAMES = ['Sihouette', 'Davies-Bouldin_Index', 'Calinski-Harabasz']


def test_every_method_is_dispatched_or_known_to_be_missing(monkeypatch):
    from deep_interpolation_clustering_amd import p2_clustering_optK as p2
    from deep_interpolation_clustering_amd import p4_clustering_final as p4
    assert len(set(cli.METHODS)) == len(cli.METHODS)
    assert set(p2.BRANCHES) <= set(cli.METHODS) and set(cli.METHODS) - set(p2.BRANCHES) == {'dl'}
    assert set(p4.Cluster.BRANCHES) <= set(cli.METHODS) and set(cli.METHODS) - set(p4.Cluster.BRANCHES) == {'optics'}
    seen = []
    real = argparse.ArgumentParser.add_argument
    monkeypatch.setattr(argparse.ArgumentParser, 'add_argument', lambda self, *a, **kw: seen.append((a[0], kw.get('choices'))) or real(self, *a, **kw))
    for program in (p2, p4):
        del seen[:]
        program.get_arguments([])
        assert dict(seen)['--cluster_method'] == cli.METHODS
        assert dict(seen)['--outlier_contamination'] is None and program.get_arguments(['--outlier_contamination', '0.1']).outlier_contamination == 0.1
    assert p2.contamination_arg is cli.contamination_arg and p4.contamination_arg is cli.contamination_arg


@pytest.mark.gpu
def test_metric_values():
    import torch
    from deep_interpolation_clustering_amd import cluster_stats
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.normal(0.0, 1.0, (32, 4)), rng.normal(3.0, 1.0, (32, 4))]).astype(np.float32)
    labels = np.repeat(np.arange(2, dtype=np.int64), 32)
    Xd = torch.as_tensor(X, device='cuda')

    def direct(x, lab):
        return [cluster_stats.silhouette_score(x, lab), cluster_stats.davies_bouldin_score(x, lab), cluster_stats.calinski_harabasz_score(x, lab)]
    metrics = cli.build_metrics(NAMES)
    np.testing.assert_allclose(cli.metric_values(Xd, labels, metrics), direct(X, labels), rtol=1e-12, atol=0)
    # the caller's pair pass is used as it is, and the Dunn index gets the min / max terms it needs from the helper's own
    stats = cluster_stats.pair_stats(Xd, labels, need_min=False, need_max=False)
    np.testing.assert_allclose(cli.metric_values(Xd, labels, metrics, stats=stats), direct(X, labels), rtol=1e-12, atol=0)
    np.testing.assert_allclose(cli.metric_values(Xd, labels, cli.build_metrics(['Dunn_Index'] + NAMES)),
                               [cluster_stats.dunn_index(X, labels)] + direct(X, labels), rtol=1e-12, atol=0)
    # --metric_sample: the draw of RandomState(0) over the labels given; a sample no smaller than the labelling is the whole labelling
    pick = np.random.RandomState(0).choice(64, 16, replace=False)
    assert len(set(labels[pick])) == 2
    np.testing.assert_allclose(cli.metric_values(Xd, labels, metrics, metric_sample=16), direct(X[pick], labels[pick]), rtol=1e-12, atol=0)
    np.testing.assert_allclose(cli.metric_values(Xd, labels, metrics, metric_sample=64), direct(X, labels), rtol=1e-12, atol=0)
    # one cluster: an error, as in the kmeans, ward, kmedoids and densitypeaks branches, unless the caller asks for NaN (gmm, spectral, meanshift)
    one = np.zeros(64, dtype=np.int64)
    for sample in (0, 16):
        with pytest.raises(ValueError, match='Number of labels is 1'):
            cli.metric_values(Xd, one, metrics, metric_sample=sample)
        assert np.isnan(cli.metric_values(Xd, one, metrics, metric_sample=sample, nan_below_two=True)).all()
    assert np.isnan(cli.metric_values(Xd[:0], one[:0], metrics, nan_below_two=True)).all()
    assert len(cli.metric_values(Xd, one, metrics, nan_below_two=True)) == len(metrics)
    np.testing.assert_allclose(cli.metric_values(Xd, labels, metrics, nan_below_two=True), direct(X, labels), rtol=1e-12, atol=0)
