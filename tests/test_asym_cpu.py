"""CPU: the oracles at asymmetric arm, chain, cost and time-step parameters.

Every other parity test runs at the reference's one shipped parameter point, where m1 = m2, l1 = l2, lc1 = lc2, the
cost's two lengths, the halves of each weight pair and every link of a chain are equal: an exchange of any two of
them changes no output there.  Here
  * the yardsticks (oracle/mppi_oracle.py, the C oracle, the chain oracle at n = 2) are pinned to the reference run
    at two asymmetric parameter sets (tests/golden/make_golden_asym.py);
  * the inputs the GPU tests use at those sets are shown to have teeth: each single exchange moves the fp64 cost by
    far more than the tolerance the GPU tests hold;
  * the chain oracle is checked at non-uniform links against a Lagrangian that shares nothing with its
    coefficients(), and the C chain oracle against the NumPy one.
"""
import dataclasses
import math

import numpy as np
import pytest

import chain_oracle as CO
import coracle
import mppi_oracle as O
from helpers import (ASYM_CASES, ASYM_LINK_CASES, ASYM_STEPS, arm_of, asym_cfg, asym_chain_inputs,
                     asym_obstacle_problem, asym_problem, load_asym_loop, load_asym_step)

LINK_COUNTS = (2, 3, 4, 5, 6, 7)
W, TW = [0.5, 0.5, 5.0, 5.0], [5.0, 5.0, 50.0, 50.0]


# ---------------------------------------------------------------- the parameter sets

def _conditioning(p):
    """min over q2 of det M / (M11 M22) of control.py:241-246."""
    c2 = np.cos(np.linspace(-np.pi, np.pi, 20001))
    a = p.m2 * p.lc2 ** 2 + p.l2
    M12 = p.m2 * p.l1 * p.lc2 * c2 + a
    M11 = p.m1 * p.lc1 ** 2 + p.l1 + p.m2 * (p.l1 ** 2 + p.lc2 ** 2 + 2 * p.l1 * p.lc2 * c2) + p.l2
    return float(np.min((M11 * a - M12 ** 2) / (M11 * a)))


@pytest.mark.parametrize("name", ASYM_STEPS)
def test_parameter_sets_are_asymmetric_and_no_worse_conditioned_than_the_default(name):
    arm = arm_of(load_asym_step(name), O.ArmParams)
    v = dataclasses.astuple(arm)
    assert len(set(v)) == len(v)                                    # every constant differs from every other
    assert _conditioning(arm) >= _conditioning(O.ArmParams())
    g = load_asym_step(name)
    for w in (g["stage_cost_weight"], g["terminal_cost_weight"]):
        assert len(set(w.tolist())) == 4
    assert float(g["delta_t"]) != 0.006 and g["sigma"][0, 1] != 0.0 and g["sigma"][0, 0] != g["sigma"][1, 1]


def test_fixture_poses_are_where_they_should_be(paths):
    path = paths["xydq_circle"]
    ee = {}
    for name in ASYM_STEPS:
        g = load_asym_step(name)
        q = g["x0"]
        ee[name] = np.array([g["fk_l1"] * math.cos(q[0]) + g["fk_l2"] * math.cos(q[0] + q[1]),
                             g["fk_l1"] * math.sin(q[0]) + g["fk_l2"] * math.sin(q[0] + q[1])])
        assert np.all(g["x0"][2:] != 0.0)
    a, c = load_asym_step("a_k128_t20"), load_asym_step("c_elbowup_k128_t20")
    off = np.abs(ee["a_k128_t20"] - path[0, :2])
    assert np.all((off >= 0.01 - 1e-12) & (off <= 0.02 + 1e-12)) and off[0] != off[1]
    assert a["x0"][1] < 0 < c["x0"][1]                               # elbow-down, elbow-up
    centre = np.array([0.8, 0.8])
    assert np.any(np.sign(ee["a_k128_t20"] - centre) != np.sign(ee["c_elbowup_k128_t20"] - centre))
    assert 200 < int(c["prev_idx"]) < path.shape[0] - 200


# ---------------------------------------------------------------- the oracles reproduce the reference

def _oracle(g, paths, cls=O.OracleController, **kw):
    opt = dict(delta_t=float(g["delta_t"]), ref_path=paths["xydq_circle"], horizon_step_T=int(g["T"]),
               number_of_samples_K=int(g["K"]), param_exploration=float(g["param_exploration"]),
               param_lambda=float(g["param_lambda"]), param_alpha=float(g["param_alpha"]), sigma=g["sigma"],
               stage_cost_weight=g["stage_cost_weight"], terminal_cost_weight=g["terminal_cost_weight"],
               visualize_optimal_traj=bool(g["visualize_optimal_traj"]))
    if "u_min" in g:
        opt.update(u_min=g["u_min"], u_max=g["u_max"])
    return cls(**opt, **kw)


@pytest.mark.parametrize("name", ASYM_STEPS)
def test_numpy_oracle_matches_reference(name, paths):
    """test_oracle_golden.py's tolerances."""
    g = load_asym_step(name)
    kw = dict(obstacles=g["obstacles"], obstacle_cost=float(g["obstacle_cost"])) if "obstacles" in g else {}
    c = _oracle(g, paths, arm=arm_of(g, O.ArmParams), visualze_sampled_trajs=bool(g["sampled"]), **kw)
    c.prev_waypoints_idx = int(g["prev_idx"])
    c.u_prev = g["u_prev"].copy()
    u0, u_seq, opt, samp = c.calc_control_input(g["x0"], epsilon=g["eps"].astype(np.float64))
    L = c.last
    assert np.max(np.abs(L["S"] - g["S"]) / np.abs(g["S"])) < 1e-14
    assert int(np.argmin(L["S"])) == int(np.argmin(g["S"]))
    np.testing.assert_allclose(L["w"], g["w"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(L["w_eps_raw"], g["w_eps_raw"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(L["w_eps_filt"], g["w_eps_filt"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(L["u_new"], g["u_new"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(u_seq, g["u_seq"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(u0, g["u0"], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(opt, g["optimal_traj"], rtol=1e-13, atol=1e-14)
    if "sampled_traj" in g:
        np.testing.assert_allclose(samp[g["sampled_idx"]], g["sampled_traj"], rtol=1e-12, atol=1e-14)
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    if float(np.sum(g["w"] ** 2)) > 0.999999 and "u_min" not in g:  # one-hot weights: bit-exact update
        assert np.array_equal(L["u_new"], g["u_new"])
    if "obstacles" in g:
        r = O.rollout_costs(g["x0"], g["u_prev"], g["eps"].astype(np.float64), paths["xydq_circle"],
                            int(g["prev_idx_after"]), float(g["delta_t"]), float(g["param_lambda"]),
                            float(g["param_alpha"]), g["sigma"], g["stage_cost_weight"], g["terminal_cost_weight"],
                            float(g["param_exploration"]), arm_of(g, O.ArmParams), lo=g["u_min"], hi=g["u_max"],
                            discs=g["obstacles"], obstacle_cost=float(g["obstacle_cost"]), details=True)
        assert np.array_equal(r["flag"], g["flag"])
        np.testing.assert_allclose(r["clear"], g["clearance"], rtol=1e-9, atol=1e-13)
        assert np.max(np.abs(r["S_track"] - g["S_free"]) / np.abs(g["S_free"])) < 1e-14


@pytest.mark.parametrize("name", [n for n in ASYM_STEPS if "clamp" not in n])
def test_c_oracle_matches_reference(name, paths):
    """The C oracle has neither torque limits nor discs: every fixture without them."""
    g = load_asym_step(name)
    prev, K = int(g["prev_idx_after"]), int(g["K"])
    S = coracle.rollout_costs(g["x0"], g["u_prev"], g["eps"], paths["xydq_circle"][prev:prev + 30], float(g["delta_t"]),
                              float(g["param_lambda"]), float(g["param_alpha"]), g["sigma"], g["stage_cost_weight"],
                              g["terminal_cost_weight"], arm_of(g, O.ArmParams),
                              k_exploit=math.ceil((1 - float(g["param_exploration"])) * K))
    assert np.max(np.abs(S - g["S"]) / np.abs(g["S"])) < 1e-13
    _, w_eps = coracle.weighted_noise(S, g["eps"], float(g["param_lambda"]))
    np.testing.assert_allclose(w_eps, g["w_eps_raw"], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", ASYM_STEPS)
def test_chain_oracle_at_n2_matches_reference(name, paths):
    """test_chain_oracle.py's tolerances; the chain has no discs, so the fixture with discs is compared on the cost
    without them (S_free) alone."""
    g = load_asym_step(name)
    c = _oracle(g, paths, cls=CO.ChainOracleController, chain=CO.ChainParams.from_arm2(arm_of(g, O.ArmParams)))
    c.u_prev = g["u_prev"].copy()
    c.prev_waypoints_idx = int(g["prev_idx"])
    _, u_seq, opt, _ = c.calc_control_input(g["x0"], epsilon=g["eps"].astype(np.float64))
    S, want = c.last["S"], g["S_free"] if "obstacles" in g else g["S"]
    assert float(np.max(np.abs(S - want) / np.abs(want))) < 1e-13
    assert c.prev_waypoints_idx == int(g["prev_idx_after"])
    if "obstacles" not in g:
        assert int(np.argmin(S)) == int(np.argmin(g["S"]))
        assert float(np.max(np.abs(u_seq - g["u_seq"]))) < 1e-10 * max(1.0, float(np.max(np.abs(g["u_seq"]))))
        np.testing.assert_allclose(opt, g["optimal_traj"], rtol=1e-10, atol=1e-10)


def test_closed_loop_oracle(paths):
    """run.py:48-71 tick by tick at set a (plant utils.py:14-38 at delta_t / 2) on the fixture's noise."""
    g = load_asym_loop("k64_t20")
    arm = arm_of(g, O.ArmParams)
    c = O.OracleController(ref_path=paths["xydq_circle"], horizon_step_T=int(g["T"]), number_of_samples_K=int(g["K"]),
                           arm=arm, **asym_cfg(g))
    c.u_prev = g["u_init"].copy()
    c.prev_waypoints_idx = int(g["prev_idx0"])
    assert len(set(g["prev_idx"].tolist())) >= 3                     # the index moves along the path
    dtp = float(g["dt_plant"])
    q, dq = g["states"][0][:2].copy(), g["states"][0][2:].copy()
    state = np.concatenate([q, dq])
    for i in range(int(g["ticks"])):
        np.testing.assert_allclose(state, g["states"][i], rtol=1e-9, atol=1e-11)
        u, u_seq, _, _ = c.calc_control_input(state, epsilon=g["eps"][i].astype(np.float64))
        np.testing.assert_allclose(u, g["u"][i], rtol=1e-9, atol=1e-9)
        assert np.max(np.abs(c.last["S"] - g["S"][i]) / np.abs(g["S"][i])) < 1e-9
        assert c.prev_waypoints_idx == int(g["prev_idx"][i])
        dq = dq + dtp * O.arm_dynamic(q, dq, u, arm)
        q = q + dtp * dq
        state = np.concatenate([q, dq])
    np.testing.assert_allclose(state, g["final_state"], rtol=1e-9, atol=1e-11)


# ---------------------------------------------------------------- the arm cases have teeth

def _swap(w, i, j):
    w = np.array(w, dtype=np.float64)
    w[[i, j]] = w[[j, i]]
    return w


def arm_mutants(arm, cfg):
    """{name: (arm, cfg)} of every single exchange a kernel could make unnoticed at the symmetric defaults."""
    r, sw, tw = dataclasses.replace, cfg["stage_cost_weight"], cfg["terminal_cost_weight"]
    return {
        "m1<->m2": (r(arm, m1=arm.m2, m2=arm.m1), cfg),
        "l1<->l2": (r(arm, l1=arm.l2, l2=arm.l1), cfg),
        "lc1<->lc2": (r(arm, lc1=arm.lc2, lc2=arm.lc1), cfg),
        "fk1<->fk2": (r(arm, fk_l1=arm.fk_l2, fk_l2=arm.fk_l1), cfg),
        "fk:=l": (r(arm, fk_l1=arm.l1, fk_l2=arm.l2), cfg),
        "l:=fk": (r(arm, l1=arm.fk_l1, l2=arm.fk_l2), cfg),
        "stage 0<->1": (arm, {**cfg, "stage_cost_weight": _swap(sw, 0, 1)}),
        "stage 2<->3": (arm, {**cfg, "stage_cost_weight": _swap(sw, 2, 3)}),
        "terminal 0<->1": (arm, {**cfg, "terminal_cost_weight": _swap(tw, 0, 1)}),
        "terminal 2<->3": (arm, {**cfg, "terminal_cost_weight": _swap(tw, 2, 3)}),
        "stage<->terminal": (arm, {**cfg, "stage_cost_weight": tw, "terminal_cost_weight": sw}),
        "dt:=0.006": (arm, {**cfg, "delta_t": 0.006}),
        "Sigma:=diag": (arm, {**cfg, "sigma": np.diag(np.diag(cfg["sigma"]))}),
    }


@pytest.mark.parametrize("name,K,T", ASYM_CASES)
def test_arm_cases_have_teeth(name, K, T, paths):
    """Each mutant moves the fp64 cost of the case's inputs by a median >= 1e-3 relative: 20 times the GPU tests'
    tolerance on S.  The noise is NumPy's with the case's Sigma (the GPU tests draw Philox noise of the same
    covariance); 200 samples settle a median."""
    g, cfg, x0, prev, u = asym_problem(name, T)
    arm = arm_of(g, O.ArmParams)
    eps = np.random.default_rng(5).multivariate_normal(np.zeros(2), cfg["sigma"], (200, T)).astype(np.float32)

    def cost(a, c):
        return O.rollout_costs(x0, u, eps.astype(np.float64), paths["xydq_circle"], prev, c["delta_t"],
                               c["param_lambda"], c["param_alpha"], c["sigma"], c["stage_cost_weight"],
                               c["terminal_cost_weight"], c["param_exploration"], a)

    S = cost(arm, cfg)
    moved = {k: float(np.median(np.abs(cost(a, c) - S) / np.abs(S))) for k, (a, c) in arm_mutants(arm, cfg).items()}
    print(name, K, T, {k: f"{v:.1e}" for k, v in moved.items()})
    assert min(moved.values()) >= 1e-3, moved


def test_obstacle_case_has_teeth(paths):
    """The discs of the GPU obstacle tests (helpers.asym_obstacle_problem) on NumPy noise: 10-90 % of the samples
    collide, and with the two lengths exchanged the masks differ on at least 10 % of the samples."""
    for K, T in ((1000, 9), (300, 20)):
        g, cfg, x0, prev, u = asym_problem("a_k128_t20", T)
        arm = arm_of(g, O.ArmParams)
        eps = np.random.default_rng(6).multivariate_normal(np.zeros(2), cfg["sigma"], (K, T)).astype(np.float32)
        p = asym_obstacle_problem(g, cfg, x0, prev, u, eps.astype(np.float64), paths)
        q, discs = p["free"]["q"], p["discs"]
        masks = {}
        for key, (a, b) in {"true": (arm.fk_l1, arm.fk_l2), "swapped": (arm.fk_l2, arm.fk_l1)}.items():
            dist, _ = O.segment_test(np.cos(q[..., 0]), np.sin(q[..., 0]), np.cos(q.sum(-1)), np.sin(q.sum(-1)), discs, a, b)
            masks[key] = O.touch_mask(dist, discs)
        share = float(np.mean((masks["true"] != 0).any(1)))
        differ = float(np.mean((masks["true"] != masks["swapped"]).any(1)))
        print(f"K {K} T {T}: {share:.1%} collide, masks differ on {differ:.1%} with the lengths exchanged")
        assert 0.10 <= share <= 0.90 and differ >= 0.10
        hit = masks["true"]
        assert np.any(hit & 1) and not np.any(hit & (3 << 2))        # link 1's end touches disc 0; nothing disc 1


# ---------------------------------------------------------------- the chain oracle from first principles

def _lagrangian_qdd(q, dq, v, P):
    """Joint accelerations of the planar chain from its Lagrangian, with nothing taken from CO.coefficients: the
    mass matrix from the centre-of-mass Jacobians plus I on the absolute rates and J on the joint rates, the
    potential from the centre-of-mass heights, dM/dq and dV/dq by central differences (h = 1e-6), the Christoffel
    terms, and the damping b dq."""
    n = P.n
    m, l, lc, I, J, b = (np.asarray(getattr(P, f), dtype=np.float64) for f in ("m", "l", "lc", "I", "J", "b"))

    def com(qq):
        th = np.cumsum(qq)
        joint = np.concatenate([[0.0 + 0.0j], np.cumsum(l * np.exp(1j * th))])[:-1]
        return joint + lc * np.exp(1j * th), th

    def mass(qq):
        th = np.cumsum(qq)
        M = np.diag(J).astype(np.float64)
        for k in range(n):
            # d(com_k)/dq_j = sum over the links i >= j up to k of i * (length along link i to com_k) e^{i th_i}
            Jc = np.zeros(n, dtype=complex)
            for j in range(k + 1):
                seg = sum(l[i] * 1j * np.exp(1j * th[i]) for i in range(j, k)) + lc[k] * 1j * np.exp(1j * th[k])
                Jc[j] = seg
            Jv = np.stack([Jc.real, Jc.imag])
            w = (np.arange(n) <= k).astype(np.float64)                  # d(th_k)/dq_j
            M += m[k] * (Jv.T @ Jv) + I[k] * np.outer(w, w)
        return M

    def potential(qq):
        c, _ = com(qq)
        return float(P.g * np.sum(m * c.imag))

    h = 1e-6
    M = mass(q)
    dM = np.zeros((n, n, n))                                            # dM[k] = dM / dq_k
    dV = np.zeros(n)
    for k in range(n):
        e = np.zeros(n)
        e[k] = h
        dM[k] = (mass(q + e) - mass(q - e)) / (2 * h)
        dV[k] = (potential(q + e) - potential(q - e)) / (2 * h)
    # c_i = sum_jk (dM_ij/dq_k - 1/2 dM_jk/dq_i) dq_j dq_k
    cor = np.einsum("kij,j,k->i", dM, dq, dq) - 0.5 * np.einsum("ijk,j,k->i", dM, dq, dq)
    return np.linalg.solve(M, v - b * dq - cor - dV)


@pytest.mark.parametrize("n", LINK_COUNTS)
def test_chain_dynamics_equal_a_first_principles_lagrangian(n):
    """1e-7 of max(1, |qdd|): the differencing error is ~1e-10 and the agreement measured when the case was written
    2e-9, so an index error in any per-link table (1e-3 or more) cannot pass."""
    rng = np.random.default_rng(40 + n)
    for trial in range(4):
        kw = {f: tuple(rng.uniform(lo, hi, n)) for f, (lo, hi) in
              dict(m=(0.5, 1.5), l=(0.15, 0.6), lc=(0.05, 0.3), I=(0.005, 0.1), fk=(0.1, 0.6), J=(0.01, 0.4),
                   b=(0.1, 3.0)).items()}
        P = CO.ChainParams(g=9.81 - 0.1 * trial, **kw)
        for f in kw:
            assert len(set(kw[f])) == n
        q, dq, v = rng.normal(0, 1.5, n), rng.normal(0, 2, n), rng.normal(0, 5, n)
        dt = 0.004
        qn, dqn = CO.chain_forward_dynamics(q[None], dq[None], v[None], dt, P)
        got = (dqn[0] - dq) / dt
        want = _lagrangian_qdd(q, dq, v, P)
        assert float(np.max(np.abs(got - want))) < 1e-7 * max(1.0, float(np.max(np.abs(want)))), (n, trial)
        np.testing.assert_allclose(qn[0], q + dqn[0] * dt, rtol=0, atol=1e-15)


@pytest.mark.parametrize("n,K,T,lam", ASYM_LINK_CASES)
def test_c_chain_oracle_matches_numpy_at_non_uniform_links(n, K, T, lam, paths):
    P, x0, sig, u = asym_chain_inputs(n, T, CO)
    K = 48
    eps = np.random.default_rng(n).multivariate_normal(np.zeros(n), sig, (K, T)).astype(np.float32)
    S = CO.chain_rollout_costs(x0, u, eps.astype(np.float64), paths["xydq_circle"], 40, 0.006, lam, 0.98, sig, W, TW,
                               0.25, P)
    Sc = coracle.chain_rollout_costs(x0, u, eps, paths["xydq_circle"][40:70], 0.006, lam, 0.98, sig, W, TW, P,
                                     k_exploit=int(np.ceil(0.75 * K)))
    np.testing.assert_allclose(Sc, S, rtol=1e-11)
    traj = coracle.chain_traj(x0, np.repeat(u[None], 2, 0), 0.006, P)
    np.testing.assert_allclose(traj[0], CO.chain_rollout_trajectory(x0, u, 0.006, P), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("n,K,T,lam", ASYM_LINK_CASES)
def test_chain_cases_have_teeth(n, K, T, lam, paths):
    """Rolling any one per-link vector by one position moves the fp64 cost of the GPU case's inputs by a median
    >= 2e-3: ten times the chain's p99 tolerance."""
    P, x0, sig, u = asym_chain_inputs(n, T, CO)
    for f in ("m", "l", "lc", "I", "fk", "J", "b"):
        assert len(set(getattr(P, f))) == n
    eps = np.random.default_rng(6).multivariate_normal(np.zeros(n), sig, (128, T)).astype(np.float32).astype(np.float64)

    def cost(Pm):
        return CO.chain_rollout_costs(x0, u, eps, paths["xydq_circle"], 40, 0.006, lam, 0.98, sig, W, TW, 0.0, Pm)

    S = cost(P)
    moved = {f: float(np.median(np.abs(cost(dataclasses.replace(P, **{f: tuple(np.roll(getattr(P, f), 1))})) - S)
                                / np.abs(S))) for f in ("m", "l", "lc", "I", "fk", "J", "b")}
    print(n, T, {k: f"{v:.1e}" for k, v in moved.items()})
    assert min(moved.values()) >= 2e-3, moved
    assert float(np.median(np.abs(x0[n:]))) > 0.5
