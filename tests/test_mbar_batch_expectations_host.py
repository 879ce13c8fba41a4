"""``pymbar_amd.MBARBatch`` without a GPU: its host logic (extension rows, the dedup algebra, stacked covariances, result assembly)
on the numpy stand-in of the batch handle (tests/batch_standin.py) against the reference's outputs in tests/golden/
(make_golden.py::expectations_block), and its input rules.  tests/test_gpu_mbar_batch_expectations.py runs the same fixture
check on the device."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import batch
from pymbar_amd import testsystems as ts
from pymbar_amd.utils import ParameterError
from tests.batch_standin import OracleBatch

# the two data sets of tests/test_expectations.py, regenerated from their seeds as tests/golden/make_golden.py does
DATASETS = {
    "expectations_config1.npz": lambda: ts.config1(seed=0)[:4],
    "expectations_unsampled.npz": lambda: ts.harmonic_u_kn([1, 2, 3, 4], [0.5, 1.0, 1.5, 2.0], [1000, 500, 0, 800], seed=3),
}
TOL = dict(rtol=2e-7, atol=2e-9)       # tests/test_expectations.py: the single-problem class against the same entries
TOL_SE = dict(rtol=2e-6, atol=2e-8)    # ... for the se_ entries, finite entries only


def check_against_reference(golden):
    """The two fixtures as two problems of one batch, every entry of the reference the batch class covers."""
    names = sorted(DATASETS)
    data = [DATASETS[n]() for n in names]
    gs = [golden(n) for n in names]
    xs, us, Ns = [d[0] for d in data], [d[1] for d in data], [d[2] for d in data]
    with pymbar_amd.MBARBatch(us, Ns) as mb:
        assert mb.P == 2 and list(mb.K) == [5, 4] and list(mb.N) == [5000, 2300]
        assert mb.success.all() and not mb.host_fallback.any()
        r = mb.compute_expectations(xs)
        for p, g in enumerate(gs):
            np.testing.assert_allclose(r["mu"][p], g["exp_x_mu"], **TOL)
            np.testing.assert_allclose(r["sigma"][p], g["exp_x_sigma"], **TOL)
        r = mb.compute_expectations([x ** 2 for x in xs], output="differences")
        for p, g in enumerate(gs):
            np.testing.assert_allclose(r["mu"][p], g["exp_x2_diff_mu"], **TOL)
            np.testing.assert_allclose(r["sigma"][p], g["exp_x2_diff_sigma"], **TOL)
        r = mb.compute_expectations(us, state_dependent=True)
        for p, g in enumerate(gs):
            np.testing.assert_allclose(r["mu"][p], g["exp_u_sd_mu"], **TOL)
            np.testing.assert_allclose(r["sigma"][p], g["exp_u_sd_sigma"], **TOL)
        u_new = [u[:3] * 1.1 + 0.3 for u in us]
        r = mb.compute_expectations(xs, u_kn_list=u_new)
        for p, g in enumerate(gs):
            np.testing.assert_allclose(r["mu"][p], g["exp_x_newstates_mu"], **TOL)
            np.testing.assert_allclose(r["sigma"][p], g["exp_x_newstates_sigma"], **TOL)
        r = mb.compute_perturbed_free_energies(u_new)
        for p, g in enumerate(gs):
            np.testing.assert_allclose(r["Delta_f"][p], g["pert_Delta_f"], **TOL)
            np.testing.assert_allclose(r["dDelta_f"][p], g["pert_dDelta_f"], **TOL)
        r = mb.compute_entropy_and_enthalpy()
        for p, g in enumerate(gs):
            for key in ("Delta_f", "dDelta_f", "Delta_u", "dDelta_u", "Delta_s", "dDelta_s"):
                got, want = r[key][p], g["se_" + key]
                assert got.shape == want.shape
                ok = np.isfinite(want)  # (the reference's own uncertainties can be NaN for an unsampled state)
                np.testing.assert_allclose(got[ok], want[ok], err_msg=f"problem {p} {key}", **TOL_SE)
        return mb


@pytest.fixture
def standin(monkeypatch):
    monkeypatch.setattr(batch, "DeviceBatch", OracleBatch)


def test_reference_fixtures_on_standin(standin, golden):
    mb = check_against_reference(golden)
    assert mb._h is None


def test_free_energy_differences_and_overlap_on_standin(standin, golden):
    g = golden("config1_ho_K5_N5000.npz")
    g4 = golden("ho_unsampled_K4_N2300.npz")
    with pymbar_amd.MBARBatch([g["u_kn"], g4["u_kn"]], [g["N_k"], g4["N_k"]]) as mb:
        np.testing.assert_allclose(mb.f_k[0], g["f_k"], atol=1e-9)
        np.testing.assert_allclose(mb.f_k[1], g4["f_k"], atol=1e-9)
        r = mb.compute_free_energy_differences()
        np.testing.assert_allclose(r["Delta_f"][0], g["Delta_f"], atol=1e-9)
        np.testing.assert_allclose(r["dDelta_f"][0], g["dDelta_f_svd_ew"], rtol=1e-7, atol=1e-9)
        r = mb.compute_free_energy_differences(uncertainty_method="approximate")
        np.testing.assert_allclose(r["dDelta_f"][0], g["dDelta_f_approximate"], rtol=1e-7, atol=1e-9)
        assert "dDelta_f" not in mb.compute_free_energy_differences(compute_uncertainty=False)
        ov = mb.compute_overlap()
        np.testing.assert_allclose(ov["matrix"][0], g["overlap_matrix"], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(np.real(ov["scalar"][0]), g["overlap_scalar"], rtol=1e-7, atol=1e-10)
        assert ov["eigenvalues"][1].shape == (4,)
        assert mb._h.calls["gram_w"] == 1   # (the covariance pass at f_k is made once)


def test_inner_equals_the_single_problem_inner_on_standin(standin, monkeypatch):
    """``compute_expectations_inner`` with state maps that repeat states and observables, new states and resident ones, against
    the single-problem function on the single-problem stand-in (both evaluate the same sums in numpy: 1e-9)."""
    import pymbar_amd.device
    from tests.cpu_standin import OracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", OracleMatrix)
    x0, u0, N0, _ = ts.harmonic_u_kn(np.linspace(0, 2, 4), np.linspace(1, 2, 4), [60, 0, 80, 70], seed=2)
    x1, u1, N1, _ = ts.harmonic_u_kn(np.linspace(0, 1, 3), np.ones(3), [50, 40, 30], seed=3)
    A = [np.array([x0, x0 ** 2, np.cos(x0)]), np.array([x1, x1 - 1e6])]
    maps = [np.array([[0, 0, 1, 3], [0, 1, 2, 1]]), np.array([[2, 2], [1, 0]])]
    with pymbar_amd.MBARBatch([u0, u1], [N0, N1]) as mb:
        for new in (False, True):
            u_ln = [u0[:2] * 1.1 + 0.3 if new else None, u1 * 0.9 if new else None]
            if new:
                maps = [np.array([[0, 0, 1, 1], [0, 1, 2, 1]]), maps[1]]
            got = mb.compute_expectations_inner(A, u_ln, maps, return_theta=True)
            for p, (u, N_k) in enumerate(((u0, N0), (u1, N1))):
                m = pymbar_amd.MBAR(u, N_k, initial_f_k=mb.f_k[p], solver_protocol=mb._protocol)
                want = m.compute_expectations_inner(A[p], m.u_kn if u_ln[p] is None else u_ln[p], maps[p], return_theta=True)
                assert sorted(got[p]) == sorted(want)
                for key in want:
                    assert got[p][key].shape == want[key].shape
                    np.testing.assert_allclose(got[p][key], want[key], rtol=1e-9, atol=1e-12, err_msg=f"problem {p} {key} new={new}")
                np.testing.assert_array_equal(got[p]["Amin"], want["Amin"])   # (the shift is the single-problem path's)
        # free energies only (a 1-D list of states): at resident states that takes no extension row at all, in one problem or both
        for u_ln, lists in (([None, None], [np.array([0, 2, 3, 2]), np.arange(3)]), ([None, u1 * 0.9], [np.arange(4), np.array([1, 0])])):
            calls = dict(mb._h.calls)
            got = mb.compute_expectations_inner([None, None], u_ln, lists, return_theta=True)
            assert (mb._h.calls["set_ext"] > calls["set_ext"]) == (u_ln[1] is not None)
            for p, (u, N_k) in enumerate(((u0, N0), (u1, N1))):
                m = pymbar_amd.MBAR(u, N_k, initial_f_k=mb.f_k[p], solver_protocol=mb._protocol)
                want = m.compute_expectations_inner(np.array([0]), m.u_kn if u_ln[p] is None else u_ln[p], lists[p], return_theta=True)
                assert sorted(got[p]) == sorted(want) == ["Theta", "f"]
                for key in want:
                    assert got[p][key].shape == want[key].shape and got[p][key].size > 0
                    np.testing.assert_allclose(got[p][key], want[key], rtol=1e-9, atol=1e-12, err_msg=f"problem {p} {key}, states only")
        got = mb.compute_expectations_inner([None, None], [None, None], [np.arange(4), np.arange(3)])
        assert sorted(got[0]) == ["f"] and got[0]["f"].shape == (4,)


def test_input_rules_and_messages(standin):
    u = np.zeros((3, 10))
    N_k = [3, 3, 4]
    with pytest.raises(ParameterError, match="MBARBatch needs at least one problem"):
        pymbar_amd.MBARBatch([], [])
    with pytest.raises(ParameterError, match="problem 1: K = 65"):
        pymbar_amd.MBARBatch([u, np.zeros((65, 65))], [N_k, [1] * 65])
    with pytest.raises(ParameterError, match="problem 0: The sum of all N_k"):
        pymbar_amd.MBARBatch([u], [[3, 3, 3]])
    x_n, u_kn, N4, _ = ts.harmonic_u_kn([0.0, 1.0], [1.0, 1.5], [20, 20], seed=1)
    big = ts.harmonic_u_kn(np.linspace(0, 1, 60), np.ones(60), [2] * 60, seed=1)
    with pymbar_amd.MBARBatch([u_kn, u_kn, u_kn, big[1]], [N4] * 3 + [big[2]]) as mb:
        calls = dict(mb._h.calls)
        xs = [x_n, x_n, x_n, big[0]]
        with pytest.raises(ParameterError, match="uncertainty_method"):
            mb.compute_expectations(xs, uncertainty_method="svd")
        with pytest.raises(ParameterError, match="uncertainty_method"):
            mb.compute_entropy_and_enthalpy(uncertainty_method="bootstrap")
        with pytest.raises(ParameterError, match="4 problems but 3 entries"):
            mb.compute_expectations(xs[:3])
        with pytest.raises(ParameterError, match=r"problem 2: the observable must have shape \(40,\)"):
            mb.compute_expectations([x_n, x_n, x_n[:-1], big[0]])
        with pytest.raises(ParameterError, match=r"problem 1: the observable must have shape \(2, 40\)"):
            mb.compute_expectations([u_kn, x_n, u_kn, big[1]], state_dependent=True)
        bad = x_n.copy()
        bad[7] = np.nan
        with pytest.raises(ParameterError, match="problem 1: the observable is not finite"):
            mb.compute_expectations([x_n, bad, x_n, big[0]])
        news = [u_kn * 1.1, u_kn * 1.1, u_kn[:, :-5] * 1.1, big[1][:2]]
        with pytest.raises(ParameterError, match="problem 2: the new states have 35 columns, fewer than the 40 samples"):
            mb.compute_perturbed_free_energies(news)
        with pytest.raises(ParameterError, match="problem 2: the new states have 35 columns, fewer than the 40 samples"):
            mb.compute_expectations(xs, u_kn_list=news)
        news[2] = u_kn * np.nan
        with pytest.raises(ParameterError, match="problem 2: the new states hold NaN"):
            mb.compute_perturbed_free_energies(news)
        # an augmented size above 128: K = 60 with 70 new states, or 60 states + 60 new states + 60 observables
        news[2] = u_kn
        news[3] = np.tile(big[1], (2, 1))[:70]
        with pytest.raises(ParameterError, match=r"problem 3: K \+ extra rows = 130 > 128: use MBAR"):
            mb.compute_perturbed_free_energies(news)
        news[3] = big[1] * 1.1
        with pytest.raises(ParameterError, match=r"problem 3: K \+ extra rows = 180 > 128: use MBAR"):
            mb.compute_expectations(xs, u_kn_list=news)
        with pytest.raises(ParameterError, match="problem 1: observable 0 is not finite"):
            mb.compute_expectations_inner([x_n[None], bad[None], x_n[None], big[0][None]], [None] * 4, [np.zeros((2, 1), int)] * 4)
        assert mb._h.calls == calls   # every rule above is checked before any device work
        # 60 states + 60 observables at the resident states fit
        r = mb.compute_entropy_and_enthalpy()
        assert r["Delta_u"][3].shape == (60, 60)
    mb.close()   # (a second close is harmless)
    mb.close()
    for call in (mb.compute_overlap, mb.compute_free_energy_differences, mb.compute_entropy_and_enthalpy,
                 lambda: mb.compute_expectations(xs), lambda: mb.compute_perturbed_free_energies(news)):
        with pytest.raises(ParameterError, match="the batch is closed"):
            call()


def test_entropy_and_enthalpy_refuses_infinite_potentials_up_front(standin):
    """The potentials are the observables of the decomposition: a +inf entry (legitimate in u_kn) leaves none, as for ``MBAR``."""
    x_n, u_kn, N_k, _ = ts.harmonic_u_kn([0.0, 1.0], [1.0, 1.5], [20, 20], seed=1)
    u_inf = u_kn.copy()
    u_inf[1, 3] = np.inf
    with pymbar_amd.MBARBatch([u_kn, u_inf], [N_k, N_k]) as mb:
        assert not mb.host_fallback.any()
        calls = dict(mb._h.calls)
        with pytest.raises(ParameterError, match=r"problem 1: the potentials hold \+inf: no entropy / enthalpy decomposition"):
            mb.compute_entropy_and_enthalpy()
        assert mb._h.calls == calls
        r = mb.compute_expectations([x_n, x_n])   # (everything else still answers)
        assert np.all(np.isfinite(r["mu"][1]))


def test_the_handle_is_released(standin):
    x_n, u_kn, N_k, _ = ts.harmonic_u_kn([0.0, 1.0], [1.0, 1.5], [20, 20], seed=1)
    mb = pymbar_amd.MBARBatch([u_kn], [N_k])
    h = mb._h
    assert not h.closed
    with mb:
        pass
    assert h.closed and mb._h is None
    mb = pymbar_amd.MBARBatch([u_kn], [N_k])
    h = mb._h
    del mb
    assert h.closed


def test_fallback_is_answered_by_the_single_problem_path(standin, monkeypatch):
    import pymbar_amd.device
    from tests.cpu_standin import OracleMatrix
    from tests.test_mbar_batch_host import disconnected_problem

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", OracleMatrix)
    u_d, N_d = disconnected_problem()
    x_n, u_kn, N_k, _ = ts.harmonic_u_kn([0.0, 1.0], [1.0, 1.5], [20, 20], seed=1)
    x_d = np.linspace(-1.0, 1.0, u_d.shape[1])
    with pymbar_amd.MBARBatch([u_kn, u_d], [N_k, N_d]) as mb:
        assert list(mb.host_fallback) == [False, True]
        m = pymbar_amd.MBAR(u_d, N_d, solver_protocol=mb._protocol)
        np.testing.assert_array_equal(mb.f_k[1], m.f_k)
        got = mb.compute_expectations([x_n, x_d])
        want = m.compute_expectations(x_d)
        for key in ("mu", "sigma"):
            np.testing.assert_array_equal(got[key][1], want[key])
        u_new = [u_kn * 1.1, np.array([(x_d - 0.2) ** 2, 2.0 * (x_d + 0.1) ** 2])]
        got = mb.compute_perturbed_free_energies(u_new)
        want = m.compute_perturbed_free_energies(u_new[1])
        for key in want:
            np.testing.assert_array_equal(got[key][1], want[key])
        np.testing.assert_array_equal(mb.compute_overlap()["matrix"][1], m.compute_overlap()["matrix"])
        # (the entropy / enthalpy decomposition takes the potentials as observables, and these hold +inf: the single-problem
        # path has no numbers for this problem, and the batch passes its error on)
        with pytest.raises(np.linalg.LinAlgError):
            m.compute_entropy_and_enthalpy()
        with pytest.raises(np.linalg.LinAlgError):
            mb.compute_entropy_and_enthalpy()
        m.close()
