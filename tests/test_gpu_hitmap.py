"""Hit maps on the device (chr_hitmap_accumulate through GPUHitMap and
Simulation.hit_map) against the host twin and the numpy restatement of the rule
(tests/hitmap_model.py): every word of every array, on both accumulation paths."""
import numpy as np
import pytest

import hitmap_model as hmm
from hitmap_model import NSOURCES, START, N_USED
from test_hitmap import _model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from chroma.gpu import create_cuda_context
    return create_cuda_context()


@pytest.fixture
def path(monkeypatch):
    def force(p):
        if p is None:
            monkeypatch.delenv('CHR_HITMAP_PATH', raising=False)
        else:
            monkeypatch.setenv('CHR_HITMAP_PATH', p)
    return force


def _device_maps(maps):
    from types import SimpleNamespace
    from chroma.gpu import gpuarray as ga
    return SimpleNamespace(solid_id_map=ga.to_gpu(maps.solid_id_map),
                           solid_id_to_channel_index_gpu=ga.to_gpu(maps.solid_id_to_channel_index_gpu),
                           nchannels=maps.nchannels)


def _photon_words(gp):
    got = gp.get()
    return [np.asarray(getattr(got, f)).copy().view(np.uint32)
            for f in ('t', 'flags', 'last_hit_triangles', 'weights', 'evidx', 'pos')]


@pytest.mark.parametrize('forced', ['d', 'l'])
def test_made_records(cuda, small_detector, path, forced):
    """Device == host twin == numpy for the made records, in source order and with
    evidx shuffled, with each optional array present and absent; twice; in parts."""
    from chroma import gpu
    from chroma.gpu.hitmap import DIRECT, PRIVATISED
    path(forced)
    maps = hmm.detector_maps(small_detector)
    gdet = gpu.GPUDetector(small_detector)
    for shuffled in (False, True):
        ph, _ = hmm.made_records(small_detector, shuffled=shuffled)
        gp = gpu.GPUPhotons(ph, copy_flags=True, copy_triangles=True, copy_weights=True)
        before = _photon_words(gp)
        for opt in hmm.OPTIONS:
            label = 'path %s, shuffled %d, %r' % (forced, shuffled, opt)
            want = _model(maps, ph, START, N_USED, NSOURCES, opt)
            twin = gpu.HostHitMap(maps, NSOURCES, **opt)
            twin.accumulate(ph, START, N_USED)
            hmm.assert_same_words(hmm.words_of(twin), want, label + ' (host twin)')
            hm = gpu.GPUHitMap(gdet, NSOURCES, **opt)
            assert hm.row_words <= gpu.hitmap.LDS_WORDS
            hm.accumulate(gp, START, N_USED)
            assert hm.last_path == (PRIVATISED if forced == 'l' else DIRECT), label
            hmm.assert_same_words(hmm.words_of(hm), want, label)
            hm.accumulate(gp, START, N_USED)
            twice = {a: None if want[a] is None else (want[a] if a == 'tmin' else want[a] * 2) for a in hmm.ARRAYS}
            hmm.assert_same_words(hmm.words_of(hm), twice, label + ' twice')
            hm.clear()
            hm.accumulate(gp, START, 1000)
            hm.accumulate(gp, START + 1000, 0)
            hm.accumulate(gp, START + 1000, N_USED - 1000)
            hmm.assert_same_words(hmm.words_of(hm), want, label + ' in parts')
        # the host HitMap of the last options
        got = hm.get()
        assert np.array_equal(got.counts.reshape(-1), want['counts']) and got.skipped == int(want['skipped'][0])
        for a, b in zip(before, _photon_words(gp)):
            assert np.array_equal(a, b), 'accumulate changed the photons'


@pytest.mark.parametrize('forced', ['d', 'l', None])
def test_wide_detector(cuda, path, forced):
    """4096 channels through a stand-in detector.  With 16 time bins a source's row is
    far over the LDS budget, so a forced privatised path falls back to the direct one;
    with tmin alone it is 8192 words = 32 KB, exactly the budget."""
    from chroma import gpu
    from chroma.gpu.hitmap import DIRECT, PRIVATISED, LDS_WORDS
    path(forced)
    maps, ph = hmm.wide_maps(), hmm.wide_records()
    gmaps = _device_maps(maps)
    gp = gpu.GPUPhotons(ph, copy_flags=True, copy_triangles=True, copy_weights=True)
    for opt, fits in ((dict(tbins=16, trange=(0.0, 64.0), earliest=True, weights=True), False),
                      (dict(tbins=0, trange=None, earliest=True, weights=False), True)):
        want = _model(maps, ph, 0, len(ph), hmm.WIDE_SOURCES, opt)
        hm = gpu.GPUHitMap(gmaps, hmm.WIDE_SOURCES, **opt)
        assert (hm.row_words <= LDS_WORDS) == fits
        hm.accumulate(gp)
        # unforced, counts and tmin alone go the direct way (the default privatises maps with
        # a time histogram or weight sums: test_simulation_hit_map)
        assert hm.last_path == (PRIVATISED if fits and forced == 'l' else DIRECT), (forced, opt)
        hmm.assert_same_words(hmm.words_of(hm), want, 'wide, path %s, %r' % (forced, opt))
    assert want['counts'].max() >= 2


def test_sweep_of_empty_words(cuda, small_detector, monkeypatch):
    """CHR_HITMAP_SWEEP=a (the sweep adds the words that hold nothing too): the same words."""
    from chroma import gpu
    monkeypatch.setenv('CHR_HITMAP_PATH', 'l')
    monkeypatch.setenv('CHR_HITMAP_SWEEP', 'a')
    maps = hmm.detector_maps(small_detector)
    ph, _ = hmm.made_records(small_detector, shuffled=True)
    gp = gpu.GPUPhotons(ph, copy_flags=True, copy_triangles=True, copy_weights=True)
    opt = hmm.OPTIONS[0]
    hm = gpu.GPUHitMap(gpu.GPUDetector(small_detector), NSOURCES, **opt)
    hm.accumulate(gp, START, N_USED)
    assert hm.last_path == gpu.hitmap.PRIVATISED
    hmm.assert_same_words(hmm.words_of(hm), _model(maps, ph, START, N_USED, NSOURCES, opt), 'sweep all')


@pytest.fixture(scope='module')
def flash_sim(cuda, small_detector):
    from chroma.sim import Simulation
    sim = Simulation(small_detector, seed=hmm.FLASH_SEED, nthreads_per_block=64, max_blocks=64)
    assert len(sim.rng_states) == hmm.FLASH_SLOTS
    return sim, hmm.flashes(sim.gpu_geometry.packed.material_objects)


FLASH_OPT = dict(tbins=20, trange=(0.0, 40.0), earliest=True, weights=True)


def test_after_propagate(flash_sim, small_detector, path):
    """Six flashes generated and propagated on the device, then accumulated: the map
    of the photons as they are downloaded."""
    from chroma import gpu
    sim, steps = flash_sim
    maps = hmm.detector_maps(small_detector)
    rng = gpu.get_rng_states(hmm.FLASH_SLOTS, seed=hmm.FLASH_SEED)
    made = gpu.generate_photons(steps, sim.gpu_geometry, rng)
    assert len(made) == sum(hmm.FLASH_SIZES)
    made.propagate(sim.gpu_geometry, rng, nthreads_per_block=64, max_blocks=64, max_steps=100)
    ph = made.get()
    want = _model(maps, ph, 0, len(ph), len(hmm.FLASH_SIZES), FLASH_OPT)
    assert np.array_equal(want['emitted'], np.array(hmm.FLASH_SIZES, np.uint64)) and want['skipped'][0] == 0
    both = (want['counts'].reshape(-1, 2) > 0).all(axis=1)
    assert both.sum() >= 2, 'at least two sources detect on both channels'
    for forced in ('d', 'l'):
        path(forced)
        hm = gpu.GPUHitMap(sim.gpu_geometry, len(hmm.FLASH_SIZES), **FLASH_OPT)
        hm.accumulate(made)
        hmm.assert_same_words(hmm.words_of(hm), want, 'after a propagate, path ' + forced)
    got = hm.get()
    assert np.array_equal(got.visibility()[both], got.counts[both] / np.array(hmm.FLASH_SIZES, float)[both][:, None])
    assert np.isfinite(got.tmin[both]).all() and (got.tmin[both] > 0).all()


@pytest.mark.parametrize('use_weights', [False, True])
def test_simulation_hit_map(flash_sim, small_detector, use_weights):
    """Simulation.hit_map in several batches and more than one group == the documented
    call sequence done by hand, word for word, rng_states included."""
    from chroma import gpu
    from chroma.sim import Simulation, hit_map_batches
    sim0, steps = flash_sim
    maps = hmm.detector_maps(small_detector)
    nsources = len(hmm.FLASH_SIZES)
    # three copies of the flashes, the later ones from other sources' ids: 5 batches of >= 1000 photons
    parts = []
    for k in range(3):
        part = hmm.flashes(sim0.gpu_geometry.packed.material_objects)
        part.steps['evidx'] = (part.steps['evidx'] + 2 * k) % nsources
        parts.append(part)
    records = np.concatenate([p.records(sim0.gpu_geometry.packed.material_objects) for p in parts])
    batches = hit_map_batches(records['nphotons'], 1000)
    assert len(batches) == 6 and records[batches[-1][0]:]['nphotons'].sum() == 333

    sim = Simulation(small_detector, seed=29, nthreads_per_block=64, max_blocks=64)
    sim.pipeline_batches = 4
    got = sim.hit_map(iter(parts), nsources, max_steps=100, photons_per_batch=1000, use_weights=use_weights,
                      **FLASH_OPT)
    assert sim.last_pipeline == (6, 2) and sim.last_exhausted == 0
    default = gpu.GPUHitMap(sim.gpu_geometry, nsources, **FLASH_OPT)      # the path hit_map took, unforced
    default.accumulate(gpu.GPUPhotons(hmm.made_records(small_detector)[0]))
    assert default.last_path == gpu.hitmap.PRIVATISED

    rng = gpu.get_rng_states(64 * 64, seed=29)
    want = None
    for first in (0, 4):
        made = [gpu.generate_photons(records[a:b], sim.gpu_geometry, rng) for a, b in batches[first:first + 4]]
        gpu.propagate_batches(made, sim.gpu_geometry, rng, nthreads_per_block=64, max_blocks=64, max_steps=100,
                              use_weights=use_weights)
        for m in made:
            ph = m.get()
            want = _model(maps, ph, 0, len(ph), nsources, FLASH_OPT, into=want)
    assert np.array_equal(sim.rng_states.get(), rng.get()), 'rng_states differ from the manual sequence'
    assert np.array_equal(got.counts.reshape(-1), want['counts']) and np.array_equal(got.emitted, want['emitted'])
    assert np.array_equal(got.thist.reshape(-1), want['thist']) and got.skipped == 0
    assert np.array_equal(got.wsum.reshape(-1), want['wsum'] / 2.0 ** 24)
    assert np.array_equal(got.tmin.reshape(-1).view(np.uint32), hmm.times_of(want['tmin']).view(np.uint32))
    assert got.emitted.sum() == 3 * sum(hmm.FLASH_SIZES) and got.counts.sum() > 20
    plain = want['counts'].astype(np.uint64) << np.uint64(24)
    if use_weights:
        assert (want['wsum'] != plain).any(), 'weighted propagation must leave weights that are not 1'
    else:
        assert np.array_equal(want['wsum'], plain)
