"""What the two Gaussian mixture front ends share (``_gmm_base.py``), host side (no GPU): the argument errors both classes raise, once over both, and the
draws of the initialisations against a direct restatement of scikit-learn's order on one NumPy stream."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deep_interpolation_clustering_amd.gmm import GaussianMixture
from deep_interpolation_clustering_amd.gmm_full import FullGaussianMixture

CLASSES = [GaussianMixture, FullGaussianMixture]


@pytest.mark.parametrize('cls', CLASSES)
def test_shared_argument_errors(cls):
    name = cls.__name__
    for bad in (0, -1, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='n_components must be an int >= 1, got %r' % (bad,)):
            cls(bad)
        with pytest.raises(ValueError, match='n_init must be an int >= 1, got %r' % (bad,)):
            cls(2, n_init=bad)
        with pytest.raises(ValueError, match='max_iter must be an int >= 1, got %r' % (bad,)):
            cls(2, max_iter=bad)
    with pytest.raises(ValueError, match=r'tol and reg_covar must be >= 0, got -1.0 and 1e-06'):
        cls(2, tol=-1.0)
    with pytest.raises(ValueError, match=r'tol and reg_covar must be >= 0, got 0.001 and nan'):
        cls(2, reg_covar=float('nan'))
    with pytest.raises(ValueError, match="init_params must be 'kmeans', 'k-means\\+\\+', 'random' or 'random_from_data', got 'zeros'"):
        cls(2, init_params='zeros')
    with pytest.raises(ValueError, match='n_components=33 > 32: outside the compiled limit'):
        cls(33)
    X = np.zeros((10, 8), np.float32)
    for call in ('predict', 'predict_proba', 'score_samples', 'score', 'bic', 'aic'):
        with pytest.raises(RuntimeError, match='^This %s instance is not fitted yet.$' % name):
            getattr(cls(2), call)(X)
    fitted = cls(2)
    fitted.weights_, fitted.n_features_in_, fitted._shift = np.full(2, 0.5), 9, np.zeros(9)
    with pytest.raises(ValueError, match='^X has 8 features, but %s is expecting 9 features as input.$' % name):
        fitted.predict(X)
    with pytest.raises(ValueError, match=r"The parameter 'weights' should have the shape of \(2,\), but got \(3,\)"):
        cls(2, weights_init=[0.2, 0.3, 0.5])._check_inits(8)
    for w in ([0.5, 0.6], [-0.5, 1.5]):
        with pytest.raises(ValueError, match=r"The parameter 'weights' should be in the range \[0, 1\] and normalized"):
            cls(2, weights_init=w)._check_inits(8)
    with pytest.raises(ValueError, match=r"The parameter 'means' should have the shape of \(2, 8\), but got \(3, 8\)"):
        cls(2, means_init=np.zeros((3, 8)))._check_inits(8)
    given = cls(2, weights_init=[0.25, 0.75], means_init=np.ones((2, 8)))._check_inits(8)
    assert sorted(given) == ['mu', 'w'] and given['w'].tolist() == [0.25, 0.75] and given['mu'].dtype == np.float64
    with pytest.raises(ValueError, match=r'order must be a permutation of 0..1, got \[0, 0\]'):
        cls(2).reorder([0, 0])
    with pytest.raises(NotImplementedError, match='sample is not implemented'):
        cls(2).sample(3)


def _stub_points(n=40, d=4):
    x = torch.as_tensor(np.random.RandomState(1).normal(size=(n, d)).astype(np.float32))
    return SimpleNamespace(x=x, n=n, d0=d, d=d)


@pytest.fixture
def streams(monkeypatch):
    """Every stream ``_random_state`` hands out, per class, in order."""
    made = {cls: [] for cls in CLASSES}
    for cls in CLASSES:
        real = cls._random_state
        monkeypatch.setattr(cls, '_random_state', lambda self, real=real: made[type(self)].append(real(self)) or made[type(self)][-1])
    return made


@pytest.mark.parametrize('init', ['random', 'random_from_data'])
def test_draws_follow_sklearns_order_on_one_stream(streams, init):
    """``_draw`` of both classes against scikit-learn's draws written out (``_base.py`` :98-141, once per restart): 'random' takes uniform(size=(n, K)) and
    normalises the rows, 'random_from_data' takes choice(n, size=K, replace=False) and gives row idx[k] to component k.  Afterwards the stream stands where
    the restatement's does."""
    pts, K, n_init, seed = _stub_points(), 3, 3, 5
    rs = np.random.RandomState(seed)
    if init == 'random':
        want_labels, want_resp = None, np.empty((n_init, pts.n, K))
        for r in range(n_init):
            u = rs.uniform(size=(pts.n, K))
            want_resp[r] = u / u.sum(axis=1)[:, np.newaxis]
    else:
        want_labels, want_resp = np.full((n_init, pts.n), -1, np.int32), None
        for r in range(n_init):
            want_labels[r, rs.choice(pts.n, size=K, replace=False)] = np.arange(K)
    after = rs.random_sample()
    for cls in CLASSES:
        labels, resp = cls(K, n_init=n_init, init_params=init, random_state=seed)._draw(pts, None)
        if init == 'random':
            assert labels is None and resp.dtype == torch.float64 and np.array_equal(resp.numpy(), want_resp)
        else:
            assert resp is None and labels.dtype == torch.int32 and np.array_equal(labels.numpy(), want_labels)
        assert len(streams[cls]) == 1 and streams[cls][0].random_sample() == after, cls.__name__


@pytest.mark.parametrize('cls', CLASSES)
def test_given_labels_replace_the_draws_after_the_stream_is_taken(streams, cls):
    pts = _stub_points()
    given = np.random.RandomState(2).randint(3, size=(2, pts.n))
    labels, resp = cls(3, n_init=2, random_state=7)._draw(pts, given)
    assert resp is None and labels.dtype == torch.int32 and np.array_equal(labels.numpy(), given)
    assert len(streams[cls]) == 1 and streams[cls][0].random_sample() == np.random.RandomState(7).random_sample()          # (taken, and nothing drawn)
