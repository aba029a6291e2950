"""Where the tolerances of tests/kat_cases.py come from: every closed-form case on the two CPU builds of the oracle.

``TOL = 4 x max(error of the fp64 oracle, error of the fp32 oracle)`` at 70 envs, so each build must stay below TOL / 4 here --
the table cannot be loosened for the kernels (tests/test_kat_gpu.py) without this test failing.  The fp64 error is how far the
discrete model is from the formula, the fp32 error what rounding costs a correct single-precision implementation.
"""
import pytest

import kat_cases as kc
import oracle_backend as ob


def test_every_case_has_its_tolerances():
    assert list(kc.TOL) and set(kc.TOL) == set(kc.CASES) and len(kc.CASES) == 14


@pytest.mark.parametrize('build', ['f64', 'f32'])
@pytest.mark.parametrize('case', list(kc.CASES))
def test_closed_form_on_the_oracle_builds(case, build):
    backend = ob.OracleBackend if build == 'f64' else ob.flavour(build)
    if backend is None:
        pytest.skip('oracle/%s is not built (make -C oracle builds every flavour)' % ob.FLAVOURS[build])
    assert ob.lib(backend.lib_path).dgo_real_bytes() == {'f64': 8, 'f32': 4}[build]
    r = kc.CASES[case](kc.make_env_factory(backend), 70)
    print('%s %s: %s' % (case, build, ' '.join('%s %.3g (env %d)' % (k, v, r.env[k]) for k, v in r.items())))
    assert set(r) == set(kc.TOL[case]), (set(r), set(kc.TOL[case]))
    bad = {k: 'error %.4g in env %d > %.4g = TOL / 4' % (v, r.env[k], kc.TOL[case][k] / 4) for k, v in r.items() if not v <= kc.TOL[case][k] / 4}
    assert not bad, (case, build, bad)
