"""The two Gaussian mixture front ends on the MI355X against tests/golden/gmm_frontend_parent.npz, BIT for bit: what the last commit in which ``gmm.py`` and
``gmm_full.py`` each carried their own constructor checks, draws, EM poll loop and winner rule published on an MI355X
(scripts/record_gmm_frontend_golden.py).  The shared base (``_gmm_base.py``) reorders no draw, no launch and no floating-point operation."""
import os
import runpy
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REC = SimpleNamespace(**runpy.run_path(os.path.join(HERE, os.pardir, 'scripts', 'record_gmm_frontend_golden.py')))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'gmm_frontend_parent.npz'))


def check(got, golden, prefix, n_names):
    """Every recorded array under ``prefix`` is there again, with the recorded dtype, shape and bytes (a recorded error: the same class and message)."""
    want = sorted(name for name in golden.files if name.startswith(prefix))
    assert sorted(got) == want and len(want) in (n_names, 1), (sorted(got), want)
    for name in want:
        a, b = got[name], golden[name]
        print(name, a.tolist() if a.size <= 8 else a.shape)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize('init', REC.INITS)
@pytest.mark.parametrize('family,case', REC.CASES)
def test_front_ends_equal_the_recorded_bits(golden, family, case, init):
    """n_init = 2, random_state = 3, every ``init_params``: the ten fitted attributes (``_status`` among them: iterations, stopping reason and last bound
    of both restarts), then predict, predict_proba, score_samples, score, bic and aic of the first half of the rows before and after ``reorder`` with the
    reversed permutation, and the reordered labels_.  gmm: 17 x 12 diag; 300 x 13 (padded features); a strided view read in place; spherical.  gmm_full:
    17 x 4 full; 257 x 13 full (padded); 255 x 64 tied; tied with duplicated rows."""
    check(REC.run_case(family, case, init), golden, '%s/%s/%s/' % (family, case, init), len(REC.ATTRS) + 2 * 6 + 1)


@pytest.mark.parametrize('family,case', REC.SWEEPS)
def test_sweeps_equal_the_recorded_bits(golden, family, case):
    """``gmm_sweep`` and ``gmm_full_sweep`` (tied: K = 3 reuses the total scatter matrix K = 2 formed) over K = 2, 3."""
    check(REC.run_sweep(family, case), golden, '%s/sweep_%s/' % (family, case), 2 * len(REC.ATTRS))
