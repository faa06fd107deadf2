"""The photon-library log-likelihood on the device (chr_library_loglike through
GPUPhotonLibrary.log_likelihood and chroma.likelihood.LibraryLikelihood) against the
host twin and the numpy restatement of the rule (tests/loglike_model.py): every word of
ll, bad and skipped, on both paths of the kernel, with the path taken asserted."""
import ctypes

import numpy as np
import pytest

import library_model as lm
import loglike_model as llm
from test_gpu_library import _device_library, _unchanged, cuda  # noqa: F401  (cuda: a fixture)
from test_library_loglike import entries, models, run_case, same_words  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# (channels, the path the kernel takes unforced): 2 is one partial wave; 4096 whole tiles on either path;
# 4097 leaves a workgroup with one live lane, whose reduction must see zeros from the other lanes
PATHS = [(2, 0), (300, 1), (4096, 1), (4097, 0)]


@pytest.mark.parametrize('nchannels,wide', PATHS)
def test_made_records(cuda, models, entries, nchannels, wide, monkeypatch):    # noqa: F811
    """Device == host twin == numpy on every made case (both modes, with and without times,
    the zero, tiny and infinite floors; hypotheses of 0 .. 65 entries, a run of empty ones
    last), on every path the shape admits; the library's arrays unchanged."""
    from chroma.gpu.library import NARROW, WIDE
    monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)
    made = lm.made_library(nchannels)
    lib, twin = _device_library(made), lm.host_library(made)
    for case in range(len(llm.CASES)):
        want = models(nchannels, case)
        assert same_words(run_case(twin, entries, nchannels, case).get(), want)
        for forced in ((None, 'n') if wide else (None,)):
            if forced:
                monkeypatch.setenv('CHR_LIBRARY_PATH', forced)
            got = run_case(lib, entries, nchannels, case).get()
            monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)
            timed = llm.CASES[case][1]                         # with observed times the narrow path is the only one
            assert lib.last_loglike_path == (WIDE if wide and not forced and not timed else NARROW), (nchannels, forced)
            assert same_words(got, want), 'case %d, %d channels, path %r: %r' % (
                case, nchannels, forced, (got.words - want.words, got.bad, want.bad, got.skipped, want.skipped))
    assert _unchanged(lib, made), 'log_likelihood changed the library'
    if nchannels == 300:        # a library without a time histogram
        made = lm.made_library(300, thist=False)
        assert same_words(run_case(_device_library(made), entries, 300, 0).get(), models(300, 0, thist=False))


def test_hypothesis_stride_past_the_grid(cuda):    # noqa: F811
    """65,537 one-entry hypotheses on the 2-channel library: two more than the grid's y
    limit, so the first two workgroup rows take a second hypothesis.  The hypotheses cycle
    through 60 different entries, whose words come from the model."""
    from chroma.library import LibraryEntries
    made = lm.made_library(2)
    sources = np.array([0, 1, 2, 3, 4, 5, 6, 7, lm.NSOURCES, lm.NO_SOURCE])
    combos = [(s, n, t) for s in sources for n in (0, 7, 1000) for t in (0.5, np.nan)]
    nobs, tobs = llm.made_observed(2)
    floor = np.float32(1e-3)
    tfloor = llm.default_tfloor(made, floor)
    one = LibraryEntries(np.arange(len(combos) + 1), *zip(*combos))
    want = llm.numpy_loglike(made, one, nobs, tobs, llm.POISSON, floor, tfloor)
    assert len(set(want.words.tolist())) > 10
    nhyp = 65537
    pick = (np.arange(nhyp) * 7) % len(combos)
    many = LibraryEntries(np.arange(nhyp + 1), one.source[pick], one.nphotons[pick], one.t[pick])
    got = _device_library(made).log_likelihood(many, nobs, tobs, floor=floor).get()
    twin = lm.host_library(made).log_likelihood(many, nobs, tobs, floor=floor).get()
    assert np.array_equal(got.words, want.words[pick]) and np.array_equal(twin.words, got.words)
    assert not got.bad.any() and got.skipped == twin.skipped == int((many.source >= lm.NSOURCES).sum()) > 0


@pytest.mark.parametrize('nchannels', [300, 4097])
def test_hypotheses_without_entries(cuda, nchannels, monkeypatch):    # noqa: F811
    """Empty hypotheses last and empty hypotheses alone, on both paths: the floor's words,
    and no entry index outside the table (the entry arrays are exactly as long as the
    offsets say)."""
    from test_library import trailing_empty_entries
    made = lm.made_library(nchannels)
    lib = _device_library(made)
    nobs, tobs = llm.made_observed(nchannels)
    floor = np.float32(1e-3)
    tfloor = llm.default_tfloor(made, floor)
    for label, en in trailing_empty_entries():
        want = llm.numpy_loglike(made, en, nobs, tobs, llm.POISSON, floor, tfloor)
        for forced in (None, 'n'):
            monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)
            if forced:
                monkeypatch.setenv('CHR_LIBRARY_PATH', forced)
            got = lib.log_likelihood(en, nobs, tobs, floor=floor).get()
            assert same_words(got, want), (label, forced)
        monkeypatch.delenv('CHR_LIBRARY_PATH', raising=False)


def test_outputs_are_written_not_added_to(cuda, entries):    # noqa: F811
    """d_ll and d_bad pre-filled with garbage hold the model's words after the call, and the
    same words after a second call on the same buffers; *d_skipped is added to."""
    from chroma.gpu import _native, gpuarray as ga
    from chroma.gpu.tools import current_stream
    made = lm.made_library(300)
    lib = _device_library(made)
    nobs, tobs = llm.made_observed(300)
    want = llm.numpy_loglike(made, entries, nobs, tobs, llm.POISSON, np.float32(1e-3), np.float32(1e-4))
    keep, desc = lib._upload_entries(entries)
    observed, obs = lib._observed(nobs, tobs, 'poisson', 1e-3, 1e-4)
    ll = ga.to_gpu(np.full(entries.nevents, -0x0123456789ABCDEF, np.int64))
    bad = ga.to_gpu(np.full(entries.nevents, 0xDEADBEEF, np.uint32))
    skipped = ga.to_gpu(np.full(1, 1000, np.uint64))
    for call in (1, 2):
        _native.call('chr_library_loglike', ctypes.byref(lib._desc()), ctypes.byref(desc), ctypes.byref(obs),
                     ll.gpudata, bad.gpudata, skipped.gpudata, current_stream())
        assert np.array_equal(ll.get(), want.words) and np.array_equal(bad.get(), want.bad), 'call %d' % call
        assert int(skipped.get()[0]) == 1000 + call * want.skipped
    del keep, observed


def test_sampled_inputs_stay_on_the_device(cuda):    # noqa: F811
    """The n and t of a device Sampled are scored where they are."""
    from chroma import gpu
    from chroma.gpu import gpuarray as ga
    from chroma.library import LibraryEntries
    from chroma.likelihood import LibraryLikelihood
    made = lm.made_library(300)
    lib = _device_library(made)
    truth = LibraryEntries([0, 2], [0, 3], [40, 9], [1.0, 2.5])
    drawn = lib.sample(truth, gpu.get_rng_states(300, seed=5))
    assert isinstance(drawn.n, ga.GPUArray) and isinstance(drawn.t, ga.GPUArray)
    en = lm.made_entries()
    floor = np.float32(1e-3)
    out = lib.log_likelihood(en, drawn.n, drawn.t, floor=floor)
    assert out._keep[1][0] is drawn.n and out._keep[1][1] is drawn.t, 'no copy, no download'
    n, t = drawn.n.get(), drawn.t.get()
    assert (n > 0).sum() > 10
    want = llm.numpy_loglike(made, en, n, t, llm.POISSON, floor, llm.default_tfloor(made, floor))
    assert same_words(out.get(), want)
    lik = LibraryLikelihood(lib, drawn, floor=floor)
    assert lik.n is drawn.n and lik.t is drawn.t
    assert np.array_equal(lik.eval(en), -(want.words / 2.0 ** 20))
    with pytest.raises(ValueError):
        lib.log_likelihood(en, drawn.t)                       # float32 words are no counts


# ------------------------------------------------------------------ on the 2-PMT detector
# six flashes whose visibilities differ from spot to spot by far more than their counting noise
CLOSURE_SIZES = (20000, 30000, 25000, 15000, 40000, 35000)
CLOSURE_SPOTS = ((0, 0, 0), (100, 50, -200), (-300, 0, 100), (0, 0, 400), (50, -100, 0), (0, 200, -400))


def test_exact_closure(cuda, small_detector):    # noqa: F811
    """A library of six flashes: with nobs = the counts of flash s, the hypothesis "source
    s, nphotons = emitted[s]" has w = 1, so m = nobs + floor on every channel, and scores
    strictly highest of the scan over the sources -- checked first on the host twin, with a
    margin far above the 2^-20 the words resolve; the device words are the model's."""
    from chroma import gensteps as gs
    from chroma import gpu
    from chroma.library import LibraryEntries
    from chroma.likelihood import LibraryLikelihood
    from chroma.sim import Simulation
    sim = Simulation(small_detector, seed=11, nthreads_per_block=64, max_blocks=64)
    water = [m for m in sim.gpu_geometry.packed.material_objects if getattr(m, 'name', None) == 'water'][0]
    steps = gs.Gensteps.join([gs.isotropic_flash(water, n, x0=x, evidx=i)
                              for i, (n, x) in enumerate(zip(CLOSURE_SIZES, CLOSURE_SPOTS))])
    ns = len(CLOSURE_SIZES)
    table = sim.hit_map(steps, ns, max_steps=100, tbins=20, trange=(0.0, 40.0))
    assert np.array_equal(table.emitted, np.array(CLOSURE_SIZES, np.uint64)) and (table.counts > 0).all()
    lib, twin = gpu.GPUPhotonLibrary(table), gpu.HostPhotonLibrary(table)
    made = lm.SimpleNamespace(nsources=ns, nchannels=2, tbins=20, t_lo=twin.t_lo, inv=twin.inv, **twin.words())
    floor = np.float32(1e-3)
    for s in range(ns):
        nobs = table.counts[s]
        en = LibraryEntries(np.arange(ns + 1), np.arange(ns), np.full(ns, table.emitted[s]), np.zeros(ns))
        want = llm.numpy_loglike(made, en, nobs, None, llm.POISSON, floor, 0.0)
        assert np.array_equal(want.mu[s], nobs.astype(np.float32)), 'w == 1: mu is the counts'
        host = twin.log_likelihood(en, nobs, floor=floor).get()
        assert same_words(host, want)
        margin = (host.words[s] - np.delete(host.words, s).max()) / 2.0 ** 20
        print('flash %d: counts %s, margin %.2f' % (s, nobs.tolist(), margin))
        assert margin > 1.0, 'the flashes must differ enough'
        got = lib.log_likelihood(en, nobs, floor=floor).get()
        assert same_words(got, want)
        scan = LibraryLikelihood(lib, (nobs, None), floor=floor).scan(int(table.emitted[s]))
        assert np.array_equal(scan, -(want.words / 2.0 ** 20)) and int(np.argmin(scan)) == s
        assert (np.delete(scan, s) > scan[s]).all()


def test_library_likelihood_device_equals_host(cuda):    # noqa: F811
    """LibraryLikelihood.scan and best on the device == the same calls on the host twin."""
    from chroma import event, gpu
    from chroma.library import VoxelGrid
    from chroma.likelihood import LibraryLikelihood
    made = lm.made_library(300)
    grid = VoxelGrid((0, 0, 0), (4, 2, 1), (4, 2, 1))
    dev = _device_library(made)
    dev.grid = grid
    host = gpu.HostPhotonLibrary(made, grid=grid)
    nobs, tobs = llm.made_observed(300)
    nobs = np.minimum(nobs, 50)
    ch = event.Channels(nobs > 0, np.where(nobs > 0, tobs, np.float32(1e9)).astype(np.float32), nobs.astype(np.float32))
    for mode in ('poisson', 'hit'):
        a, b = LibraryLikelihood(dev, ch, mode=mode), LibraryLikelihood(host, ch, mode=mode)
        a.group_bytes = b.group_bytes = 20 * 5                  # five hypotheses per call
        sa, sb = a.scan(40, t0=1.5), b.scan(40, t0=1.5)
        assert sa.shape == (4, 2, 1) and np.array_equal(sa, sb)
        assert a.best((40, 400), (0.0, 1.5)) == b.best((40, 400), (0.0, 1.5))
