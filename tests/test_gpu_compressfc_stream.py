"""The four row-streaming kernels of the CompressFC node (bnhead_bwd_reduce, bnhead_fwd, fc_bwd, row_proj + statistics) are held bit for bit to what the
commit before their load pipelines were deepened computed: tests/golden/compressfc_stream.json, written by tests/compressfc_stream_fixture.py on that
commit.  How rows are fetched may change; every operation and every summation order may not.  The row counts (see the fixture) put each lane's trip count
below, at and above the depth of the load ring, cross the one-workgroup / several-workgroup and the grid-cap boundaries, and end ragged."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

KERNELS = ('bnhead_fwd', 'bnhead_bwd_reduce', 'fc_bwd', 'fc_bwd_bnhead', 'row_proj_stats')


@pytest.fixture(scope='module')
def got_want(golden_dir):
    spec = importlib.util.spec_from_file_location('compressfc_stream_fixture', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'compressfc_stream_fixture.py'))
    fx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fx)
    with open(os.path.join(golden_dir, 'compressfc_stream.json')) as f:
        want = json.load(f)
    return fx.digests(), want


def test_the_fixture_covers_the_same_cases(got_want):
    got, want = got_want
    assert sorted(got) == sorted(want)
    for k in KERNELS:
        assert any(name.startswith(k + '/') for name in want), k


@pytest.mark.parametrize('kernel', KERNELS)
def test_outputs_are_the_bits_of_the_single_prefetch_kernels(got_want, kernel):
    got, want = got_want
    names = [n for n in sorted(want) if n.startswith(kernel + '/')]
    assert names
    bad = [n for n in names if got.get(n) != want[n]]
    assert not bad, '%d of %d outputs differ: %s' % (len(bad), len(names), bad[:8])
