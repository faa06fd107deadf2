"""The photon-library lookup on the device (chr_library_expect, chr_library_sample
through GPUPhotonLibrary, Simulation.build_library / simulate_library) against the
host twins and the numpy restatement of both rules (tests/library_model.py): every
word of every output and of the generator states, on both paths of the expect kernel."""
from types import SimpleNamespace

import numpy as np
import pytest

import hitmap_model as hmm
import library_model as lm
from test_library import _same_floats, models, entries, trailing_empty_entries  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


def _device_library(made):
    """A GPUPhotonLibrary over device copies of a made library's words (a stand-in for
    the GPUHitMap it adopts)."""
    from chroma import gpu
    from chroma.gpu import gpuarray as ga
    on = {k: None if getattr(made, k) is None else ga.to_gpu(getattr(made, k))
          for k in ('emitted', 'counts', 'tmin', 'thist')}
    return gpu.GPUPhotonLibrary(SimpleNamespace(nsources=made.nsources, nchannels=made.nchannels, tbins=made.tbins,
                                                t_lo=made.t_lo, inv=made.inv, **on))


def _unchanged(lib, made):
    words = lib.words()
    return all((words[k] is None and getattr(made, k) is None) or np.array_equal(words[k], getattr(made, k))
               for k in words)


# (channels, the path the expect kernel takes unforced)
PATHS = [(2, 0), (300, 1), (4096, 1), (4097, 0)]


@pytest.mark.parametrize('nchannels,wide', PATHS)
def test_expect_made_records(cuda, models, entries, nchannels, wide, monkeypatch):    # noqa: F811
    """Device == host twin == numpy: 4097 and 2 channels through the narrow path, 4096 and
    300 through the wide one and, forced, through the narrow one; each optional array absent
    (300 channels); the library's arrays unchanged."""
    from chroma.gpu.library import NARROW, WIDE
    monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)
    for tmin, thist in ([(True, True), (False, True), (True, False), (False, False)] if nchannels == 300
                        else [(True, True)]):
        made = lm.made_library(nchannels, tmin=tmin, thist=thist)
        want = models(nchannels, tmin, thist)
        twin = lm.host_library(made).expect(entries).get()
        assert _same_floats(twin.mu, want.mu)
        lib = _device_library(made)
        for forced in ((None, 'n') if wide else (None,)):
            if forced:
                monkeypatch.setenv('CHR_LIBRARY_PATH', forced)
            got = lib.expect(entries).get()
            assert lib.last_path == (WIDE if wide and not forced else NARROW), (nchannels, forced)
            assert _same_floats(got.mu, want.mu), 'mu words differ (%d channels, path %r)' % (nchannels, forced)
            assert (got.tfirst is None) == (not tmin)
            if tmin:
                assert _same_floats(got.tfirst, want.tfirst), 'tfirst words differ'
            assert got.skipped == want.skipped > 0
            monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)
        assert _unchanged(lib, made), 'expect changed the library'


@pytest.mark.parametrize('nchannels', [2, 300, 4096, 4097])
def test_sample_made_records(cuda, models, entries, nchannels):    # noqa: F811
    """Device == host twin == numpy for n, t, skipped and the generator states, with
    fewer slots than pairs, exactly as many, and more (whose states stay)."""
    from chroma import gpu
    npairs = nchannels * entries.nevents
    cases = [(n, True, True) for n in ((1, 7, npairs, npairs + 5) if nchannels == 2 else (npairs, npairs + 5))]
    if nchannels == 300:
        cases += [(npairs, False, True), (npairs, True, False), (npairs, False, False), (301, True, True)]
    for nslots, tmin, thist in cases:
        made = lm.made_library(nchannels, tmin=tmin, thist=thist)
        want = models(nchannels, tmin, thist, nslots)
        lib = _device_library(made)
        rng = gpu.get_rng_states(nslots, seed=3)
        got = lib.sample(entries, rng)
        label = '%d channels, %d slots, tmin %d, thist %d' % (nchannels, nslots, tmin, thist)
        assert np.array_equal(got.n.get(), want.n), 'n words differ: ' + label
        assert _same_floats(got.t.get(), want.t), 't words differ: ' + label
        assert int(got.skipped.get()[0]) == want.skipped > 0
        assert np.array_equal(rng.get().reshape(-1), want.states), 'rng states differ: ' + label
        assert _unchanged(lib, made), 'sample changed the library'
    channels = got.get()
    assert len(channels) == entries.nevents and channels[1].hit.dtype == bool and channels[1].q.dtype == np.float32


def test_few_slots_on_a_wide_row(cuda, entries):    # noqa: F811
    """7 slots for 2400 pairs of 300 channels: every slot walks 343 strided pairs.  Against the
    host twin (which test_library.py holds to the numpy model; the model's lane-serial rounds
    would take many seconds here)."""
    from chroma import gpu
    from chroma.gensteps import rng_init_host
    made = lm.made_library(300)
    states = rng_init_host(7, seed=3)
    want = lm.host_library(made).sample(entries, states)
    rng = gpu.get_rng_states(7, seed=3)
    got = _device_library(made).sample(entries, rng)
    assert np.array_equal(got.n.get(), want.n) and _same_floats(got.t.get(), want.t)
    assert np.array_equal(rng.get().reshape(-1), states) and int(got.skipped.get()[0]) == int(want.skipped[0]) > 0


@pytest.mark.parametrize('nchannels', [300, 4097])
def test_events_without_entries_last(cuda, nchannels, monkeypatch):
    """An event without entries as the last one, a run of them, and nothing but such events, on
    both paths: the words of the numpy model, and no entry index outside the table (the entry
    arrays are exactly as long as the offsets say)."""
    from chroma import gpu
    from chroma.gensteps import rng_init_host
    made = lm.made_library(nchannels)
    lib = _device_library(made)
    for label, en in trailing_empty_entries():
        want = lm.numpy_expect(made, en)
        for forced in (None, 'n'):
            monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)
            if forced:
                monkeypatch.setenv('CHR_LIBRARY_PATH', forced)
            got = lib.expect(en).get()
            assert _same_floats(got.mu, want.mu) and _same_floats(got.tfirst, want.tfirst), (label, forced)
            assert got.skipped == want.skipped
        monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)
        model = lm.numpy_sample(made, en, rng_init_host(64, seed=3), 64)
        rng = gpu.get_rng_states(64, seed=3)
        drawn = lib.sample(en, rng)
        assert np.array_equal(drawn.n.get(), model.n) and _same_floats(drawn.t.get(), model.t), label
        assert np.array_equal(rng.get().reshape(-1), model.states), label


# ------------------------------------------------------------------ on the 2-PMT detector
@pytest.fixture(scope='module')
def flash_sim(cuda, small_detector):
    from chroma.sim import Simulation
    sim = Simulation(small_detector, seed=hmm.FLASH_SEED, nthreads_per_block=64, max_blocks=64)
    return sim, hmm.flashes(sim.gpu_geometry.packed.material_objects)


def test_exact_closure(flash_sim):
    """A library of six flashes looked up with each source's own flash, (s, emitted[s], t):
    w is 1.0 and the counts are below 2^24, so mu is the counts and tfirst the earliest
    times, exactly; with t = 3.5 the float32 sum."""
    from chroma import gpu
    from chroma.library import LibraryEntries
    sim, steps = flash_sim
    table = sim.hit_map(steps, len(hmm.FLASH_SIZES), max_steps=100, tbins=20, trange=(0.0, 40.0))
    assert np.array_equal(table.emitted, np.array(hmm.FLASH_SIZES, np.uint64))
    assert (table.counts > 0).all(axis=1).sum() >= 2 and table.counts.max() < 2 ** 24
    lib = gpu.GPUPhotonLibrary(table)
    ns = len(hmm.FLASH_SIZES)
    for t in (0.0, 3.5):
        en = LibraryEntries(np.arange(ns + 1), np.arange(ns), table.emitted, np.full(ns, t))
        got = lib.expect(en).get()
        assert np.array_equal(got.mu, table.counts.astype(np.float32)) and got.skipped == 0
        assert _same_floats(got.tfirst, np.where(table.counts > 0, table.tmin + np.float32(t), np.float32(np.inf)))
    assert np.isfinite(got.tfirst).any() and np.isinf(got.tfirst[hmm.FLASH_SIZES.index(0)]).all()
    # a GPUHitMap's device arrays are adopted, not copied
    hm = gpu.GPUHitMap(sim.gpu_geometry, ns, tbins=4, trange=(0.0, 40.0))
    adopted = gpu.GPUPhotonLibrary(hm)
    assert all(getattr(adopted, k) is getattr(hm, k) for k in ('emitted', 'counts', 'tmin', 'thist'))


@pytest.mark.parametrize('sample', [True, False])
def test_simulate_library(cuda, small_detector, sample):
    """Simulation.simulate_library in more than one group == the documented call sequence
    done by hand, channel for channel, rng_states included."""
    from chroma import gensteps as gs
    from chroma import gpu
    from chroma.gpu.library import expected_channels
    from chroma.library import VoxelGrid, entries_from_gensteps
    from chroma.sim import Simulation
    sim = Simulation(small_detector, seed=31, nthreads_per_block=64, max_blocks=64)
    water = [m for m in sim.gpu_geometry.packed.material_objects if getattr(m, 'name', None) == 'water'][0]
    grid = VoxelGrid((-400.0, -400.0, -500.0), (400.0, 400.0, 600.0), (2, 2, 2))
    lib = sim.build_library(grid, water, 2000, tbins=20, trange=(0.0, 40.0), max_steps=100)
    assert isinstance(lib, gpu.GPUPhotonLibrary) and lib.grid is grid and lib.nsources == 8 and lib.nchannels == 2
    words = lib.words()
    assert (words['emitted'] == 2000).all() and words['counts'].sum() > 0 and words['thist'].sum() > 0
    events = [gs.isotropic_flash(water, 40000, x0=(100, 100, 100), t0=1.0)
              + gs.cherenkov_step(water, 30000, x0=(-100, 50, -200), dx=(0, 0, 30), beta=0.99, t0=2.0, dt=0.1),
              gs.Gensteps(),
              gs.isotropic_flash(water, 90000, x0=(-300, -100, 200)) + gs.isotropic_flash(water, 5, x0=(0, 0, 5000)),
              gs.scintillation_step(water, 70000, x0=(200, -200, -300), dx=(10, 0, 0), t0=-2.0)]
    sim.daq_group_bytes = 8 * 2 * 3                    # three events per group: two groups
    start = sim.rng_states.get().copy()
    got = list(sim.simulate_library(lib, iter(events), sample=sample))
    assert [ev.nphotons for ev in got] == [70000, 0, 90005, 70000]
    rng = gpu.RNGStates(64 * 64)
    rng.array.set(start.reshape(-1))
    want = []
    for group in (events[:3], events[3:]):
        en = entries_from_gensteps(grid, group)
        want += lib.sample(en, rng).get() if sample else expected_channels(lib.expect(en).get())
    assert np.array_equal(sim.rng_states.get(), rng.get()), 'rng_states differ from the manual sequence'
    assert np.array_equal(sim.rng_states.get(), start) == (not sample)
    for a, b in zip(got, want):
        assert np.array_equal(a.channels.hit, b.hit) and _same_floats(a.channels.t, b.t) \
            and _same_floats(a.channels.q, b.q)
    assert not got[1].channels.hit.any() and sum(int(ev.channels.hit.sum()) for ev in got) > 0
    # and the host twin over the downloaded words gives the same channels
    twin = gpu.HostPhotonLibrary(SimpleNamespace(nsources=8, nchannels=2, tbins=20, t_lo=lib.t_lo, inv=lib.inv, **words))
    if not sample:
        host = expected_channels(twin.expect(entries_from_gensteps(grid, events)).get())
        assert all(_same_floats(a.channels.q, b.q) and _same_floats(a.channels.t, b.t) for a, b in zip(got, host))


def test_sharded_simulation_refuses():
    from chroma.sim import ShardedSimulation
    with pytest.raises(NotImplementedError):
        ShardedSimulation.build_library(object(), None, None, 1)
    with pytest.raises(NotImplementedError):
        ShardedSimulation.simulate_library(object(), None, [])
