"""The tally rows of the registered box operators (fusion-sim_amd/csrc/fes_ops.inc.hpp): a family keeps one row of exact
integers per registered operator and one more for the call that is applied now.  Per family, MAX_OPS operators are registered
with the periods 1 .. MAX_OPS (the forces: envelopes that start at sub-step k), their requests identical except for seed and
stream; after 2 MAX_OPS sub-steps, taken one at a time with a one-shot call of the same family between two of them, row k
holds the integer sum of what a twin's one-shot calls returned in the hook's order — no row has leaked into its neighbour or
into the call's row, `applications` is the host's count, and the one-shot call returned what the twin's did.  The twin is
filled from a checkpoint and does the manual loop, as in tests/test_gpu_sequences2.py, whose helpers this module uses.
Everything is equality of exact integers or of bits: no tolerance anywhere."""
import math

import numpy as np
import pytest

import sequence_model as model
import test_gpu_sequences as g1
import test_gpu_sequences2 as g2

pytestmark = pytest.mark.gpu

SHAPE = (16, 8, 16)
L = tuple(1e-3 * s for s in SHAPE)
COUNTS = (2000, 1900)
DT = 5e-12
W = 1e15 * float(np.prod(L)) / COUNTS[0]
DV = float(np.prod(L)) / float(np.prod(SHAPE))
SCENE = dict(seed=77, solver="poisson_fft", precision="fp32", sort_interval=2, counts=list(COUNTS), masses=[model.ME, model.MP], charges=[model.QE, -model.QE],
             spec=dict(radius=L[0], length_y=L[1], height=L[2], nr=SHAPE[0], ny=SHAPE[1], nz=SHAPE[2], dt=DT, nparticles=0, count=COUNTS[0],
                       particle_mass=model.ME, particle_charge=model.QE, geometry="cart3d", solver="poisson_fft", macro_weight=W))


def _tally():
    return dict(sigma=model.fusion_table(), g_lo=model.FUSION_G[0], g_hi=model.FUSION_G[1], tau=DT)


def _gas():
    lo, hi = model.gas_compact_range()
    return dict(species=0, density=model.gas_density(math.sqrt(lo * hi), DT), tau=DT, sigma=model.gas_table(), g_lo=model.GAS_G[0], g_hi=model.GAS_G[1],
                **model.BACKGROUND)


# per family: MAX_OPS' name, the request without seed, stream and epoch, (now, register, stats) of a handle and a request, the
# count that shows an application did something
FAMILIES = {
    "collide": ("COLLIDE_MAX_OPS", lambda: dict(species=0, nu_tau=0.2, mass_ratio=2.0, **model.BACKGROUND),
                lambda s, kw: s.collide("elastic", **kw), lambda s, every, kw: s.collideEvery(every, "elastic", **kw), lambda s, k: s.collisionStats(k), "collided"),
    "gas": ("GAS_MAX_OPS", _gas,
            lambda s, kw: s.collideGas("exchange", **kw), lambda s, every, kw: s.collideGasEvery(every, "exchange", **kw), lambda s, k: s.gasStats(k), "collided"),
    "pair": ("PAIR_MAX_OPS", lambda: dict(log_lambda=model.LOG_LAMBDA, tau=model.pair_tau(W, DV, model.ME, model.QE, model.MP, -model.QE, n_l=1)),
             lambda s, kw: s.collidePair(0, 1, **kw), lambda s, every, kw: s.collidePairEvery(every, 0, 1, **kw), lambda s, k: s.pairStats(k), "pairs"),
    "fusion": ("FUSION_MAX_OPS", _tally,
               lambda s, kw: s.fusionYield(0, 1, grid=True, **kw), lambda s, every, kw: s.fusionYieldEvery(every, 0, 1, **kw),
               lambda s, k: dict(s.fusionStats(k), grid=s.fusionGrid(k)), "pairs"),
    "spectrum": ("FUSION_SPECTRUM_MAX_OPS", lambda: dict(_tally(), **model.spectrum_axis(SCENE["masses"], 0, 1, "cm")),
                 lambda s, kw: s.fusionSpectrum(0, 1, **kw), lambda s, every, kw: s.fusionSpectrumEvery(every, 0, 1, **kw), lambda s, k: s.fusionSpectrumRead(k), "pairs"),
}
FORCE = dict(kind="field", species=0, waves=[dict(amp=[3e5, -2e5, 1e5], mode=[1, 0, -2], nu=0.15, phase=0.25)], taper=[None, [0.5, 1.5, 1.0], None])


@pytest.fixture(scope="module")
def fp():
    import fusionpic
    fusionpic.load_library()
    return fusionpic


def _pair_of_handles(fp, tmp_path):
    a = g1.build(fp, SCENE)
    for sp, n in enumerate(COUNTS):
        pos, vel = model.particles(SCENE["seed"], 1000 + sp, n, lengths=L)
        a.set(position=pos, velocity=vel, species=sp)
    a.precalc()
    return a, g1.twin_of(fp, SCENE, a, tmp_path / "twin.ckpt")


def _check(a, b, stats, sums, most, done, key):
    for k in range(most):
        have = g2.ints_of(stats(a, k))
        assert g2.equal_sums(have, sums[k]) and all(key_ in have for key_ in sums[k]), (k, {x: v for x, v in have.items() if x != "grid"}, {x: v for x, v in sums[k].items() if x != "grid"})
        assert have["applications"] == done[k] > 0 and have[key] > 0, (k, have["applications"], done[k], have[key])
    assert g1.same_particles(g1.particles_of(a, SCENE), g1.particles_of(b, SCENE))


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_row_holds_its_own_operators_sums(fp, tmp_path, family):
    most_name, request, now, register, stats, key = FAMILIES[family]
    most = getattr(fp, most_name)
    a, b = _pair_of_handles(fp, tmp_path)
    kws = [dict(request(), seed=1000 + k, stream=k, epoch=40) for k in range(most)]
    for k, kw in enumerate(kws):
        assert register(a, k + 1, kw) == k
    sums = [{} for _ in range(most)]
    for t in range(1, 2 * most + 1):
        a.substeps(1)
        b.substeps(1)
        for k, kw in enumerate(kws):      # (the hook's order within a family: the registration's)
            if t % (k + 1) == 0:
                g2.add_ints(sums[k], now(b, dict(kw, epoch=t + kw["epoch"])))
        if t == most:                      # the call's own row, between two sub-steps: the twin has no registered rows beside it
            kw = dict(request(), seed=4242, stream=31, epoch=t)
            got, want = now(a, kw), now(b, kw)
            assert g2.exact(got) == g2.exact(want) and got["applications"] == 1 and got[key] > 0, (got, want)
    _check(a, b, stats, sums, most, [2 * most // (k + 1) for k in range(most)], key)
    a.destroy()
    b.destroy()


def test_every_row_holds_its_own_forces_sums(fp, tmp_path):
    """a force has no period: request k is active from sub-step k on (s = the handle's own count of sub-steps + epoch, and a
    checkpoint carries no count: the twin's count is A's)"""
    most = fp.FORCE_MAX_OPS
    a, b = _pair_of_handles(fp, tmp_path)
    kws = [dict(FORCE, envelope=dict(start=k)) for k in range(most)]
    for k, kw in enumerate(kws):
        assert a.forceOn(**kw) == k
    sums = [{} for _ in range(most)]
    for t in range(1, 2 * most + 1):
        a.substeps(1)
        b.substeps(1)
        for k, kw in enumerate(kws):
            g2.add_ints(sums[k], b.force(**kw))
        if t == most:
            kw = dict(FORCE, species=1, epoch=3)
            got, want = a.force(**kw), b.force(**kw)
            assert g2.exact(got) == g2.exact(want) and got["applications"] == 1 and got["kicked"] > 0, (got, want)
    _check(a, b, lambda s, k: s.forceStats(k), sums, most, [2 * most - max(k, 1) + 1 for k in range(most)], "kicked")
    a.destroy()
    b.destroy()
