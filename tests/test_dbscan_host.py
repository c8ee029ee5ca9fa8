"""CPU checks of the DBSCAN pieces that need no GPU: the eps -> squared-distance threshold rule and the ABI's argument checks."""
import ctypes
import os

import numpy as np
import pytest

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd.dbscan import DBSCAN, sq_threshold


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


@pytest.mark.parametrize('eps', [0.3, np.float64(0.3), 0.5, np.float64(2.5), 1.9, np.float32(0.7), 1e-3, 123.456])
def test_threshold_is_the_largest_square_under_eps(eps):
    t = np.float32(sq_threshold(eps))
    assert np.sqrt(t) <= eps
    assert not np.sqrt(np.nextafter(t, np.float32(np.inf))) <= eps


def test_threshold_follows_the_eps_type():
    # a Python float compares in f32 (f32(0.3) <= 0.3), an np.float64 in f64 (it is not)
    s = np.float32(0.3)
    assert np.float32(sq_threshold(0.3)) >= s * s
    assert np.float32(sq_threshold(np.float64(0.3))) < s * s


def test_unsupported_options():
    with pytest.raises(NotImplementedError, match='pass the points'):
        DBSCAN(0.5, metric='precomputed')
    with pytest.raises(NotImplementedError):
        DBSCAN(0.5, metric='manhattan')
    with pytest.raises(ValueError):
        sq_threshold(0.0)


def test_abi_rejects_bad_arguments_without_gpu(lib):
    thr = (ctypes.c_float * 1)(1.0)
    nb = ctypes.c_int64(0)
    fake = ctypes.c_void_p(1 << 20)          # never dereferenced: every check fails before a launch
    ws = lib.dic_dbscan_workspace(1000, 256)
    assert ws > 0 and lib.dic_dbscan_workspace(1000, 260) == 0
    # NULL pointers
    assert lib.dic_dbscan_counts(None, 256, fake, 1000, 256, thr, 1, fake, fake, 16, ctypes.byref(nb), fake, ws, None) == -1
    assert lib.dic_dbscan_counts(fake, 256, fake, 1000, 256, thr, 1, None, fake, 16, ctypes.byref(nb), fake, ws, None) == -1
    assert b'NULL' in lib.dic_last_error_string()
    # D > 256, D % 4, too many eps
    assert lib.dic_dbscan_counts(fake, 260, fake, 1000, 260, thr, 1, fake, fake, 16, ctypes.byref(nb), fake, ws, None) == -2
    assert lib.dic_dbscan_counts(fake, 256, fake, 1000, 250, thr, 1, fake, fake, 16, ctypes.byref(nb), fake, ws, None) == -2
    assert lib.dic_dbscan_counts(fake, 256, fake, 1000, 256, thr, 17, fake, fake, 16, ctypes.byref(nb), fake, ws, None) == -2
    # short workspace
    assert lib.dic_dbscan_counts(fake, 256, fake, 1000, 256, thr, 1, fake, fake, 16, ctypes.byref(nb), fake, ws - 1, None) == -3
    assert lib.dic_dbscan_components_pass(1000, 256, 1.0, 0, fake, 5, fake, 0, fake, fake, fake, fake, ws - 1, None) == -3
    assert lib.dic_dbscan_components_pass(1000, 256, 1.0, 0, None, 5, fake, 0, fake, fake, fake, fake, ws, None) == -1
    assert lib.dic_dbscan_components_pass(1000, 264, 1.0, 0, fake, 5, fake, 0, fake, fake, fake, fake, ws, None) == -2
