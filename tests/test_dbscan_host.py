"""CPU checks of the DBSCAN pieces that need no GPU: the eps -> squared-distance threshold rule, the ABI's argument checks and the register allocation of
csrc/dic_dbscan.hip."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from deep_interpolation_clustering_amd import _native as N
from deep_interpolation_clustering_amd.dbscan import DBSCAN, dbscan_sweep, sq_threshold


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
    with pytest.raises(ValueError, match='below 2\\^50'):          # before any GPU work: the padding points' norm bounds the thresholds
        dbscan_sweep(np.zeros((8, 4), np.float32), [0.5, 2.0 ** 50], 2)


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
    # a threshold too near the padding points' norm: 2^100 and above
    big = (ctypes.c_float * 1)(2.0 ** 100)
    assert lib.dic_dbscan_counts(fake, 256, fake, 1000, 256, big, 1, fake, fake, 16, ctypes.byref(nb), fake, ws, None) == -2
    assert lib.dic_dbscan_components_pass(1000, 256, 2.0 ** 100, 0, fake, 5, fake, 0, fake, fake, fake, fake, ws, None) == -2
    # short workspace
    assert lib.dic_dbscan_counts(fake, 256, fake, 1000, 256, thr, 1, fake, fake, 16, ctypes.byref(nb), fake, ws - 1, None) == -3
    assert lib.dic_dbscan_components_pass(1000, 256, 1.0, 0, fake, 5, fake, 0, fake, fake, fake, fake, ws - 1, None) == -3
    assert lib.dic_dbscan_components_pass(1000, 256, 1.0, 0, None, 5, fake, 0, fake, fake, fake, fake, ws, None) == -1
    assert lib.dic_dbscan_components_pass(1000, 264, 1.0, 0, fake, 5, fake, 0, fake, fake, fake, fake, ws, None) == -2


# ScratchSize [bytes/lane] of the five tile kernels: what the file compiled to when it moved onto dic_pairtile.h (before that, with its own copy of the loop and
# column masks in the counting epilogue: 212, 108, 172, 1232 and 44).  The product loop holds 128 accumulators + 72 operand registers of 256; the band test's
# compare masks are what the allocator still cannot place.
TILE_KERNEL_SCRATCH = {'db_count_kernelILi1E': 0, 'db_count_kernelILi4E': 76, 'db_count_kernelILi10E': 172, 'db_count_kernelILi16E': 336, 'db_label_kernel': 44}


def test_dbscan_kernels_scratch_does_not_grow():
    """A ratchet on the scratch memory of dic_dbscan.hip (dic_pairtile.h included), compiled with the Makefile's flags: none for the kernels outside the tile
    loop, and no more than TILE_KERNEL_SCRATCH for the tile kernels."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, 'deep_interpolation_clustering_amd', 'csrc')
    res = subprocess.run([hipcc, '-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-I' + os.path.join(root, 'include'), '-c',
                          os.path.join(src, 'dic_dbscan.hip'), '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    names = re.findall(r'Function Name: (\S+)', res.stderr)
    scratch = [int(v) for v in re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', res.stderr)]
    assert len(scratch) == len(names)
    seen = set()
    for name, got in zip(names, scratch):
        key = [k for k in TILE_KERNEL_SCRATCH if k in name]
        assert len(key) <= 1, name
        seen.update(key)
        assert got <= (TILE_KERNEL_SCRATCH[key[0]] if key else 0), (name, got)
    assert seen == set(TILE_KERNEL_SCRATCH), names
    assert len(names) >= len(TILE_KERNEL_SCRATCH) + 6, names          # + planes, block maxima, padding norm, recheck, band link, pointer jump
