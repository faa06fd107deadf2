"""Live records (shade_kernel's LIVE, CHR_LIVE_RECORDS): the device-driven
one-step slots of the default variant carry a surviving photon's state from
step to step in a dense 64-byte record per queue position and write the photon
arrays only when the photon dies or something else reads them next (the tail
kernel, the caller, a resumed or aliased propagate).  It is a change of where
the state travels, not of what is computed: the default must give the same
words as CHR_LIVE_RECORDS=0 (the array path) in every photon field and every
RNG slot state, and both must meet the oracle under test_gpu_batches' parity
contract -- flags and last hits exact, floats within 1e-5 * max(|oracle|, 1),
RNG states equal.

The 2-PMT detector at launch shape (64, 64) has 4,096 slots and a tail
threshold of 8,192 photons.  Its black walls absorb 95% of an isotropic point
source in the first step (the oracle leaves 1,420 of 30,000 alive), so the
30,000 / 30,001 / 9,000-photon batches run one one-step slot and then the tail
(max_steps = 2: a second one-step slot, the last step being one whatever its
length, which reads the first's 1.4k survivors from records and flushes), or at
(256, 64), below its threshold of 32,768, the tail at once.  The batches of 640,000 and
640,001 (no multiple of 64) are the ones that read records: the oracle's
survivors are 29.9k, 19.4k, 11.5k and 8.7k, so slots 1 to 4 read records, each
thread looping over up to 8 queue positions, and slot 5 is the tail; max_steps
of 2 to 5 end on a one-step slot (the flush with no next slot).  The physics
scene keeps 18.3k and 11.4k of 30,000 alive (two record slots), scint.tiny()
31k and 8.9k of 150,000.
"""
import numpy as np
import pytest

import oracle
import scenes
from test_gpu_batches import FIELDS

pytestmark = pytest.mark.gpu

SWITCH = 'CHR_LIVE_RECORDS'
FLOATS = ('pos', 'dir', 'pol', 'wavelengths', 't', 'weights')
DEAD = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 3) | (1 << 15)


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    torch.cuda.set_device(0)


def _same(a, b, label):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if x.dtype == np.float32:     # the same words (NaN included)
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), '%s: %s differs' % (label, f)


def _oracle_contract(got, host, label):
    """test_gpu_batches' contract; a NaN of the oracle must be a NaN here
    (test_gpu_photon_inputs' reading of it for photons that abort)."""
    for f in ('flags', 'last_hit_triangles'):
        assert np.array_equal(getattr(got, f), getattr(host, f)), '%s: %s differs from the oracle' % (label, f)
    for f in FLOATS:
        a = getattr(got, f).astype(np.float64)
        b = getattr(host, f).astype(np.float64)
        ok = (np.abs(a - b) <= 1e-5 * np.maximum(np.abs(b), 1.0)) | (np.isnan(a) & np.isnan(b))
        assert ok.all(), '%s: %s beyond 1e-5 of the oracle at %s' % (label, f, np.flatnonzero(~ok.ravel())[:5])


def _propagate(geom, photons, shape, max_steps, seed, use_weights=False, ncopies=1):
    """One GPUPhotons.propagate from fresh RNG states: (photons, RNG states, stats)."""
    from chroma import gpu
    rng = gpu.get_rng_states(shape[0] * shape[1], seed=seed)
    gp = gpu.GPUPhotons(photons, ncopies=ncopies, copy_flags=True, copy_triangles=True, copy_weights=True)
    gp.propagate(geom, rng, nthreads_per_block=shape[0], max_blocks=shape[1], max_steps=max_steps,
                 use_weights=use_weights)
    return gp.get(), rng.get(), gp.last_stats


def _oracle(packed, photons, shape, max_steps, seed):
    nslots = shape[0] * shape[1]
    states = oracle.rng_init(nslots, seed=seed)
    host = oracle.HostPhotons(photons)
    oracle.propagate(packed, host, states, nslots, shape[0], shape[1], max_steps)
    return host, states.reshape(6, nslots)


def _check_counter(stats, label):
    if stats.trace_launches >= 2:
        assert stats.live_record_slots == stats.trace_launches - 1, label


# ------------------------------------------------------- default vs switch, oracle
_det = {}


def _small(small_detector):
    if 'gpu' not in _det:
        from chroma import gpu
        _det['gpu'] = gpu.GPUDetector(small_detector)
    return _det['gpu']


_sources = {}


def _source(n):
    from chroma.photon_source import isotropic
    if n not in _sources:
        _sources[n] = isotropic(n, seed=100 + n % 7)
    return _sources[n]


_default_runs = {}


def _default_run(small_detector, shape, n, max_steps):
    key = (shape, n, max_steps)
    if key not in _default_runs:
        _default_runs[key] = _propagate(_small(small_detector), _source(n), shape, max_steps, seed=13)
    return _default_runs[key]


CASES = [(shape, n, ms) for shape in ((64, 64), (256, 64)) for n in (30000, 30001, 9000)
         for ms in (1, 2, 3, 7, 1000)]
ISSUE_CASES = list(CASES)
CASES += [((64, 64), n, ms) for n in (640000, 640001) for ms in (2, 3, 5, 7, 1000)]
# the oracle's share of a 640k case is 20 s; its one multi-slot case here is 200,001 photons
# (9.3k after the first step: slot 1 reads records, then the tail), the others are the scenes'
CASES += [((64, 64), 200001, 1000)]
ORACLE_CASES = ISSUE_CASES + [((64, 64), 200001, 1000)]
ONE_STEP_SLOTS_640K = 5      # 640k, 29.9k, 19.4k, 11.5k, 8.7k photons; then 5.8k < 8,192: the tail


@pytest.mark.parametrize('shape,n,max_steps', CASES)
def test_default_equals_switch(cuda, small_detector, monkeypatch, shape, n, max_steps):
    label = 'shape %s, %d photons, max_steps %d' % (shape, n, max_steps)
    monkeypatch.delenv(SWITCH, raising=False)
    got, rng, st = _default_run(small_detector, shape, n, max_steps)
    _check_counter(st, label)
    if n >= 640000:
        assert st.trace_launches == min(max_steps, ONE_STEP_SLOTS_640K), label
        assert st.live_record_slots == st.trace_launches - 1 >= 1, label
    elif n == 200001:
        assert st.trace_launches == 2 and st.live_record_slots == 1 and st.tail_photons > 0, label
    elif shape == (64, 64):
        # one slot above the threshold; the second is the tail unless it is the last step (a
        # one-step slot whatever its length: it reads the 1.4k records of the first's survivors)
        assert st.trace_launches == min(max_steps, 2 if max_steps == 2 else 1), label
        assert (st.tail_photons > 0) == (max_steps > 2), label
    if shape == (256, 64) and max_steps > 1:
        assert st.trace_launches == 0 and st.live_record_slots == 0, label
    monkeypatch.setenv(SWITCH, '0')
    off, rng_off, st_off = _propagate(_small(small_detector), _source(n), shape, max_steps, seed=13)
    assert st_off.live_record_slots == 0, label
    assert st_off.trace_launches == st.trace_launches and st_off.tail_photons == st.tail_photons, label
    _same(got, off, label)
    assert np.array_equal(rng, rng_off), label + ': RNG states differ'


@pytest.mark.parametrize('shape,n,max_steps', ORACLE_CASES)
def test_default_meets_oracle(cuda, small_detector, small_packed, monkeypatch, shape, n, max_steps):
    label = 'oracle: shape %s, %d photons, max_steps %d' % (shape, n, max_steps)
    monkeypatch.delenv(SWITCH, raising=False)
    got, rng, _ = _default_run(small_detector, shape, n, max_steps)
    host, states = _oracle(small_packed, _source(n), shape, max_steps, seed=13)
    _oracle_contract(got, host, label)
    assert np.array_equal(rng, states), label + ': RNG states differ'


def test_counter_zero_where_off(cuda, small_detector, monkeypatch):
    """No slot reads records host-driven (CHR_HOST_STEPS=1) or with use_weights
    (whose first slot is the tail); both give the default's photons where they
    run the same physics."""
    monkeypatch.delenv(SWITCH, raising=False)
    got, rng, st = _default_run(small_detector, (64, 64), 640000, 1000)
    assert st.live_record_slots >= 2
    monkeypatch.setenv('CHR_HOST_STEPS', '1')
    host_steps, rng_h, st_h = _propagate(_small(small_detector), _source(640000), (64, 64), 1000, seed=13)
    assert st_h.live_record_slots == 0 and st_h.trace_launches == st.trace_launches
    _same(got, host_steps, 'CHR_HOST_STEPS=1')
    assert np.array_equal(rng, rng_h)
    monkeypatch.delenv('CHR_HOST_STEPS')
    _, _, st_w = _propagate(_small(small_detector), _source(30000), (64, 64), 1000, seed=13, use_weights=True)
    assert st_w.live_record_slots == 0 and st_w.tail_photons == 30000


# ------------------------------------------------------------------ batches
def _batch_run(det, srcs, pattern, copies, batched, max_steps):
    from chroma import gpu
    names = sorted(set(pattern))
    rng = gpu.get_rng_states(64 * 64, seed=9)
    gps = {k: gpu.GPUPhotons(srcs[k], ncopies=copies[k], copy_flags=True, copy_triangles=False, copy_weights=False)
           for k in names}
    seq = [gps[k] for k in pattern]
    if batched:
        stats = gpu.propagate_batches(seq, det, rng, nthreads_per_block=64, max_blocks=64, max_steps=max_steps)
    else:
        stats = []
        for gp in seq:
            gp.propagate(det, rng, nthreads_per_block=64, max_blocks=64, max_steps=max_steps)
            stats.append(gp.last_stats)
    return {k: gps[k].get() for k in names}, rng.get(), stats


@pytest.mark.parametrize('pattern,copies', [('aa', 1), ('aba', 1), ('ab', 3)])
def test_batches(cuda, small_detector, monkeypatch, pattern, copies):
    """propagate_batches with batches that share photon arrays ('aa', 'aba': the
    later batch reads what the earlier one's flush and deaths wrote) and with
    ncopies > 1: batched == sequential == the switch off."""
    from chroma.photon_source import isotropic
    det = _small(small_detector)
    names = sorted(set(pattern))
    srcs = {k: isotropic((300000 if copies == 1 else 100000) + 7001 * i, seed=5 + i) for i, k in enumerate(names)}
    ncop = {k: copies for k in names}
    out = {}
    for live in (True, False):
        if live:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, '0')
        for batched in (False, True):
            out[live, batched] = _batch_run(det, srcs, pattern, ncop, batched, 7)
    ref = out[False, False]
    for key, (photons, rng, stats) in out.items():
        label = '%s x%d live=%s batched=%s' % (pattern, copies, key[0], key[1])
        for k in names:
            _same(photons[k], ref[0][k], label + ' ' + k)
        assert np.array_equal(rng, ref[1]), label
        for s in stats:
            assert s.live_record_slots == (max(0, s.trace_launches - 1) if key[0] else 0), label
    assert sum(s.live_record_slots for s in out[True, True][2]) >= 2 * len(names)


# ------------------------------------------------- non-fresh inputs, other kernels
_geo = {}


def _geometry(name):
    """(packed, GPUGeometry) of the wire-plane physics scene (the WIRES
    instantiation of the shade kernels) or demo.scint.tiny() (re-emission,
    surface models)."""
    if name not in _geo:
        from chroma import gpu, loader
        from chroma.demo import scint
        from chroma.gpu.packing import PackedGeometry
        geo = loader.create_geometry_from_obj(scenes.physics_scene() if name == 'scene' else scint.tiny())
        _geo[name] = (PackedGeometry(geo), gpu.GPUGeometry(geo))
    return _geo[name]


def _three_way(name, photons, legs, seed, monkeypatch, label, min_live_slots):
    """The legs (max_steps each, the same photons and RNG run on) by default,
    with the switch off and on the oracle: default == switch off (words), and
    the oracle's contract after every leg."""
    from chroma import gpu
    packed, gg = _geometry(name)
    nslots = 64 * 64
    host = oracle.HostPhotons(photons)
    states = oracle.rng_init(nslots, seed=seed)
    runs = {}
    for live in (True, False):
        if live:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, '0')
        gp = gpu.GPUPhotons(photons, copy_flags=True, copy_triangles=True, copy_weights=True)
        rng = gpu.get_rng_states(nslots, seed=seed)
        after = []
        for max_steps in legs:
            gp.propagate(gg, rng, nthreads_per_block=64, max_blocks=64, max_steps=max_steps)
            after.append((gp.get(), rng.get(), gp.last_stats))
        runs[live] = after
    for i, max_steps in enumerate(legs):
        oracle.propagate(packed, host, states, nslots, 64, 64, max_steps)
        got, rng, st = runs[True][i]
        off, rng_off, st_off = runs[False][i]
        leg = '%s leg %d' % (label, i)
        _same(got, off, leg)
        assert np.array_equal(rng, rng_off), leg
        _oracle_contract(got, host, leg)
        assert np.array_equal(rng, states.reshape(6, nslots)), leg + ': RNG states differ from the oracle'
        _check_counter(st, leg)
        assert st_off.live_record_slots == 0
    assert sum(r[2].live_record_slots for r in runs[True]) >= min_live_slots, label
    return host


def test_resume(cuda, monkeypatch):
    """3 steps, then the rest, on the physics scene: the first leg ends on a
    one-step slot (its survivors flushed with no next slot), the second starts
    from those arrays with most of its queue dead on entry."""
    photons = scenes.photon_sources(30000, seed=61)
    host = _three_way('scene', photons, (3, 40), 61, monkeypatch, 'resume', 2)
    assert ((host.flags & DEAD) != 0).mean() > 0.9


def test_pre_terminated(cuda, monkeypatch):
    """test_gpu_photon_inputs' terminal inputs, tiled to 72,000 photons (24,000
    alive on entry, 14.7k and 9.5k after the first steps): two in three dead on
    entry with times, weights and last hits a write would disturb; slot 0 leaves
    them alone and no record is made of them."""
    from test_gpu_photon_inputs import _terminal_photons
    from chroma.event import Photons
    p, dead, _ = _terminal_photons()
    reps = 8
    tile = lambda a: np.concatenate([a] * reps)   # noqa: E731
    photons = Photons(tile(p.pos), tile(p.dir), tile(p.pol), tile(p.wavelengths), t=tile(p.t),
                      last_hit_triangles=tile(p.last_hit_triangles), flags=tile(p.flags), weights=tile(p.weights))
    dead = tile(dead)
    host = _three_way('scene', photons, (30,), 65, monkeypatch, 'pre-terminated', 1)
    for f in ('t', 'weights', 'last_hit_triangles', 'flags'):
        assert np.array_equal(getattr(host, f)[dead], getattr(photons, f)[dead])


@pytest.mark.parametrize('name', ['scene', 'scint'])
def test_other_instantiations(cuda, monkeypatch, name):
    """The wire-plane scene (shade_kernel's WIRES form) and demo.scint.tiny()
    (re-emission, every surface model) from fresh photons."""
    from chroma.photon_source import isotropic
    photons = scenes.photon_sources(30000, seed=71) if name == 'scene' else isotropic(150000, seed=72)
    _three_way(name, photons, (1000,), 73, monkeypatch, name, 2)


# ------------------------------------------------------- switch-table conventions
def test_switch_identical(cuda, small_detector, monkeypatch):
    """('CHR_LIVE_RECORDS', '0') through test_gpu_batches.test_switches_identical's check."""
    from test_gpu_batches import test_switches_identical
    test_switches_identical(None, small_detector, monkeypatch, SWITCH, '0')
