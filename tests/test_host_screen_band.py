"""k_screen's float evaluation of the hybrid surface's network term (cm::icnn_value_f, host build) against the package's fp64
forward pass: the error bound it returns -- the band within which the screen hands a point to the double evaluation -- must
hold at every point, for every network class the library accepts ([6, H, 1], H <= 256, any weights).  A point outside the band
is stored as elastic without ever reaching the Newton solve, so a band that is too narrow misclassifies plastic points."""
import ctypes as C

import numpy as np
import pytest

import wide_hybrid as wh


def _value_f(desc, s6):
    import host_harness_lib as hh
    L = hh.lib()
    s6 = np.ascontiguousarray(s6, dtype=np.float64)
    n = s6.shape[0]
    nf, band = np.zeros(n), np.zeros(n)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L.hh_icnn_value_f(C.byref(desc), C.c_int64(n), vp(s6), vp(nf), vp(band))
    return nf, band


def _setup(net, seed=0):
    from cmad_amd.models.device import HybridHillEffectiveStress, build_desc
    from cmad_amd.synthetic import AL7079_HILL
    icnn, values = wh.wide_hybrid_setup(net[0], net[1], net[2], seed=seed, out_narrow=net[3])
    desc, info = build_desc(values, hybrid=HybridHillEffectiveStress(icnn))
    desc.nn_weights = info["nn_packed"].ctypes.data                     # the host build reads host memory (info keeps it alive)
    return icnn, values, desc, info, AL7079_HILL


@pytest.mark.parametrize("net", wh.NETWORKS, ids=wh.net_id)
def test_screen_band_bounds_the_float_network_term(net):
    icnn, values, desc, info, hill = _setup(net)
    Y = values["plastic"]["flow stress"]["initial yield"]["Y"]
    rng = np.random.default_rng(7)
    d = wh.random_deviators(2000, rng)
    d /= wh.hill_phi(d, hill)[:, None]                                     # Hill-equivalent stress 1
    s_rand = d[:1000] * (Y * rng.uniform(0.1, 3.0, 1000))[:, None]          # 0.1 ... 3 times yield
    t = wh.surface_scales(icnn, hill, Y, d[1000:])
    assert np.isfinite(t).mean() > 0.9
    s_surf = d[1000:][np.isfinite(t)] * t[np.isfinite(t), None]           # on the hybrid surface phi_hill + NN = Y
    for what, s6 in (("random", s_rand), ("surface", s_surf)):
        nf, band = _value_f(desc, s6)
        ref = wh.network_term(icnn, s6)
        err = np.abs(nf - ref)
        assert np.isfinite(nf).all() and (band > 0.0).all(), what
        assert (err <= band).all(), f"{what}: float error {err.max():.3g} MPa beyond the band at {(err > band).sum()} of " \
                                    f"{len(err)} points (worst ratio {(err / band).max():.3g})"
        if what == "surface":                                              # (on the reference's own surface)
            assert np.abs(wh.hill_phi(s6, hill) + ref - Y).max() < 1e-9 * Y


def test_screen_band_on_the_configs3_batch_sends_few_wavefronts_to_the_double_path():
    """The bound must not be so generous that the screen loses its point: on the first 2^20 points of bench.py's seeded
    configs[3] batch (hybrid_update, gauss_point_batch seed 22, x_prev = 0) the share of 64-point groups with a point inside the
    band -- a wavefront that takes the double evaluation -- may not exceed twice what the former relative band
    2e-4 (|phi_hill| + |NN| + Y + H) sent there."""
    from cmad_amd.synthetic import gauss_point_batch
    icnn, values, desc, info, hill = _setup(wh.AL7079)
    n = 1 << 20
    G = gauss_point_batch(n, seed=22, eps_y=525.0 / 70.2e3).T.reshape(n, 3, 3)
    e = 0.5 * (G + G.transpose(0, 2, 1))
    s = 2.0 * desc.mu * e + desc.lmbda * np.trace(e, axis1=1, axis2=2)[:, None, None] * np.eye(3)
    s6 = np.stack([s[:, 0, 0], s[:, 0, 1], s[:, 0, 2], s[:, 1, 1], s[:, 1, 2], s[:, 2, 2]], axis=1)
    nf, band = _value_f(desc, s6)
    ph = wh.hill_phi(s6, hill)
    YH = desc.Y                                                            # alpha = 0: Voce H(0) = 0
    dist = np.abs(ph + nf - YH)
    tol = desc.yield_tol * 2.0 * desc.mu
    group = lambda inside: inside.reshape(-1, 64).any(axis=1).mean()
    before = group(~(dist > 2e-4 * (ph + np.abs(nf) + YH)))
    after = group(~(dist > band + tol))
    print(f"64-point groups through the double evaluation: {before:.4%} with the relative band, {after:.4%} with the bound; "
          f"median bound {np.median(band):.3g} MPa")
    assert after <= 2.0 * before + 1.0 / len(dist) * 64
