"""The photon-library log-likelihood (chr_library_loglike, GPUPhotonLibrary /
HostPhotonLibrary.log_likelihood, chroma.likelihood.LibraryLikelihood) as far as it can
be checked without a GPU: the exports, every refusal (made before anything is read
through a pointer, the outputs untouched), the host twin -- library.h's rule built by the
host compiler -- against the numpy restatement of tests/loglike_model.py on every word of
ll, bad and skipped, the equalities that tie the rule to chr_library_expect, Gibbs'
inequality, and the Python layer over the host twin."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import library_model as lm
import loglike_model as llm

CHR_OK, CHR_ERR_INVALID = 0, 1
FAKE = 0x1000


# ------------------------------------------------------------------ exports and refusals
def test_entry_points_are_exported():
    from chroma import gpu
    from chroma.gpu import _native
    from chroma.likelihood import LibraryLikelihood
    l = ctypes.CDLL(_native.library_path())
    for name in ('chr_library_loglike', 'chr_library_loglike_host', 'chr_library_loglike_last_path'):
        assert name in _native.EXPORTED and hasattr(l, name)
    ret, args = _native._SIGNATURES['chr_library_loglike']
    assert ret is ctypes.c_int32 and len(args) == 7 and args[2] is ctypes.POINTER(_native.LibraryObservedDesc)
    assert len(_native._SIGNATURES['chr_library_loglike_host'][1]) == 6
    assert _native._SIGNATURES['chr_library_loglike_last_path'] == (ctypes.c_int32, [])
    fields = [(n, t) for n, t in _native.LibraryObservedDesc._fields_]
    assert fields == [('nobs', ctypes.c_void_p), ('tobs', ctypes.c_void_p), ('mode', ctypes.c_uint32),
                      ('floor', ctypes.c_float), ('tfloor', ctypes.c_float)]
    assert gpu.GPUPhotonLibrary.log_likelihood and gpu.HostPhotonLibrary.log_likelihood and LibraryLikelihood


ENTRIES = ('chr_library_loglike', 'chr_library_loglike_host')


def _call(entry, null=(), nevents=0, nsources=8, nchannels=2, ntbins=4, inv=0.5, thist=FAKE, tobs=FAKE, mode=0,
          floor=1e-3, tfloor=0.0):
    """An entry point with made-up addresses: every refusal comes before the first
    dereference or launch, and nevents == 0 touches nothing, so none is used."""
    from chroma.gpu import _native
    arg = lambda name, value=FAKE: None if name in null else value      # noqa: E731
    desc = _native.HitMapDesc(nsources, nchannels, ntbins, 0.0, inv, arg('emitted'), arg('counts'), None, thist, None,
                              None)
    en = _native.LibraryEntriesDesc(nevents, arg('offsets'), arg('source'), arg('nphotons'), arg('t'))
    ob = _native.LibraryObservedDesc(arg('nobs'), tobs, mode, floor, tfloor)
    args = (None if 'desc' in null else ctypes.byref(desc), None if 'entries' in null else ctypes.byref(en),
            None if 'obs' in null else ctypes.byref(ob), arg('ll'), arg('bad'), arg('skipped'))
    return getattr(_native.lib(), entry)(*(args if entry.endswith('_host') else args + (None,)))


@pytest.mark.parametrize('entry', ENTRIES)
def test_no_hypotheses_is_ok(entry):
    # the arguments every refusal below starts from are themselves accepted
    assert _call(entry) == CHR_OK
    assert _call(entry, ntbins=0, thist=None, tobs=None) == CHR_OK
    assert _call(entry, tobs=None, mode=1, floor=0.0, tfloor=float('inf')) == CHR_OK
    assert _call(entry, null=('offsets', 'source', 'nphotons', 't')) == CHR_OK      # not looked at without hypotheses
    assert _call(entry, nchannels=2 ** 20, nsources=1, ntbins=0, thist=None, tobs=None) == CHR_OK


@pytest.mark.parametrize('entry', ENTRIES)
def test_refusals(entry):
    from chroma.gpu import _native
    err = lambda: _native.lib().chr_last_error()      # noqa: E731
    for null in ('desc', 'entries', 'obs', 'emitted', 'counts', 'nobs', 'll', 'bad', 'skipped'):
        assert _call(entry, null=(null,)) == CHR_ERR_INVALID and b'null' in err(), null
    for null in ('offsets', 'source', 'nphotons', 't'):
        assert _call(entry, null=(null,), nevents=1) == CHR_ERR_INVALID and b'null' in err(), null
    # what chr_library_expect refuses of the library and the table
    assert _call(entry, thist=None, tobs=None) == CHR_ERR_INVALID and b'histogram' in err()
    assert _call(entry, ntbins=0) == CHR_ERR_INVALID and b'histogram' in err()
    assert _call(entry, nsources=0) == CHR_ERR_INVALID
    assert _call(entry, nchannels=0) == CHR_ERR_INVALID and _call(entry, nchannels=-2) == CHR_ERR_INVALID
    for inv in (0.0, -0.5, float('inf'), float('nan')):
        assert _call(entry, inv=inv) == CHR_ERR_INVALID and b'inv' in err()
    assert _call(entry, nsources=2 ** 31 + 1, nchannels=1, ntbins=0, thist=None, tobs=None) == CHR_ERR_INVALID
    assert b'2^31' in err()
    assert _call(entry, nsources=2 ** 16, nchannels=2 ** 15, ntbins=2) == CHR_ERR_INVALID
    assert _call(entry, nevents=2 ** 30 + 1, nchannels=2) == CHR_ERR_INVALID and b'events' in err()
    # and what only the log-likelihood refuses
    assert _call(entry, mode=2) == CHR_ERR_INVALID and b'mode' in err()
    for bad in (-1e-3, float('nan'), -float('inf')):
        assert _call(entry, floor=bad) == CHR_ERR_INVALID and b'floor' in err()
        assert _call(entry, tfloor=bad) == CHR_ERR_INVALID and b'floor' in err()
    assert _call(entry, ntbins=0, thist=None) == CHR_ERR_INVALID and b'observed times' in err()      # tobs, no thist
    assert _call(entry, nchannels=2 ** 20 + 1, nsources=1, ntbins=0, thist=None, tobs=None) == CHR_ERR_INVALID
    assert b'2^20' in err()


def _host_call(lib, en, nobs, tobs, mode, floor, tfloor, ll, bad, skipped, offsets=None):
    from chroma.gpu import _native
    desc = _native.LibraryEntriesDesc(en.nevents, (en.offsets if offsets is None else offsets).ctypes.data,
                                      en.source.ctypes.data, en.nphotons.ctypes.data, en.t.ctypes.data)
    ob = _native.LibraryObservedDesc(nobs.ctypes.data, None if tobs is None else tobs.ctypes.data, mode, floor, tfloor)
    return _native.lib().chr_library_loglike_host(ctypes.byref(lib._desc()), ctypes.byref(desc), ctypes.byref(ob),
                                                  ll.ctypes.data, bad.ctypes.data, skipped.ctypes.data)


def test_refusals_leave_the_outputs_untouched():
    """Each refusal from an otherwise accepted call on real arrays: ll, bad and skipped
    keep their words; so do they for descending offsets, which only the host twin refuses."""
    from chroma.gpu import _native
    made = lm.made_library(2)
    lib, en = lm.host_library(made), lm.made_entries()
    nobs, tobs = llm.made_observed(2)
    ll, bad, skipped = np.full(en.nevents, -7, np.int64), np.full(en.nevents, 9, np.uint32), np.full(1, 5, np.uint64)
    untouched = lambda: (ll == -7).all() and (bad == 9).all() and skipped[0] == 5      # noqa: E731
    for mode, floor, tfloor in ((2, 1e-3, 0.0), (0, -1.0, 0.0), (0, float('nan'), 0.0), (0, 1e-3, -1.0),
                                (1, 1e-3, float('nan'))):
        assert _host_call(lib, en, nobs, tobs, mode, floor, tfloor, ll, bad, skipped) == CHR_ERR_INVALID
        assert untouched()
    flat = lm.host_library(lm.made_library(2, thist=False))
    assert _host_call(flat, en, nobs, tobs, 0, 1e-3, 0.0, ll, bad, skipped) == CHR_ERR_INVALID and untouched()
    down = en.offsets.copy()
    down[3] = down[2] - 1
    assert _host_call(lib, en, nobs, tobs, 0, 1e-3, 0.0, ll, bad, skipped, offsets=down) == CHR_ERR_INVALID
    assert b'ascending' in _native.lib().chr_last_error() and untouched()
    assert _host_call(lib, en, nobs, tobs, 0, 1e-3, 0.0, ll, bad, skipped) == CHR_OK      # the accepted call
    assert not untouched() and skipped[0] > 5


# ------------------------------------------------------------------ the host twin against numpy
@pytest.fixture(scope='module')
def entries():
    return llm.trailing_empty(lm.made_entries())


@pytest.fixture(scope='module')
def models(entries):
    """The numpy model's words, computed once per case and shared (left unchanged)."""
    cache = {}

    def get(nchannels, case, thist=True):
        key = (nchannels, case, thist)
        if key not in cache:
            mode, timed, floor, tfloor = llm.CASES[case]
            made = lm.made_library(nchannels, thist=thist)
            nobs, tobs = llm.made_observed(nchannels)
            if tfloor is None:
                tfloor = llm.default_tfloor(made, floor)
            cache[key] = llm.numpy_loglike(made, entries, nobs, tobs if timed else None, mode, floor, tfloor)
        return cache[key]
    return get


def run_case(lib, entries, nchannels, case):
    """A made case through a library's log_likelihood (host twin or device)."""
    mode, timed, floor, tfloor = llm.CASES[case]
    nobs, tobs = llm.made_observed(nchannels)
    return lib.log_likelihood(entries, nobs, tobs if timed else None, mode=('poisson', 'hit')[mode], floor=floor,
                              tfloor=tfloor)


def same_words(got, want):
    return np.array_equal(got.words, want.words) and got.words.dtype == np.int64 \
        and np.array_equal(got.bad, want.bad) and got.skipped == want.skipped


@pytest.mark.parametrize('nchannels', lm.CHANNELS)
def test_host_twin_matches_numpy(models, entries, nchannels):
    lib = lm.host_library(lm.made_library(nchannels))
    before = lib.words()
    for case in range(len(llm.CASES)):
        got, want = run_case(lib, entries, nchannels, case).get(), models(nchannels, case)
        assert same_words(got, want), 'case %d: %r' % (case, (got.words - want.words, got.bad, want.bad))
        assert want.skipped > 0 and np.array_equal(got.ll, want.words / 2.0 ** 20)
    after = lib.words()
    assert all(before[k] is None or np.array_equal(before[k], after[k]) for k in before)
    # a library without a time histogram: the cases without observed times
    flat = lm.host_library(lm.made_library(nchannels, thist=False))
    for case in (0, 2):
        assert same_words(run_case(flat, entries, nchannels, case).get(), models(nchannels, case, thist=False))


def test_made_records_exercise_what_they_claim(models, entries):
    """On the numpy model alone."""
    sizes = tuple(np.diff(entries.offsets.astype(np.int64)))
    assert sizes == lm.EVENT_SIZES + (0, 0, 0), 'a run of hypotheses without entries comes last'
    made = lm.made_library(300)
    assert made.emitted[lm.UNLIT] == 0 and not made.counts.reshape(lm.NSOURCES, -1)[lm.DARK].any()
    nobs, tobs = llm.made_observed(300)
    assert nobs.max() == 2 ** 24 + 1 and (nobs == 0).sum() > 100 and np.isnan(tobs).any()
    assert np.isposinf(tobs).any() and np.isneginf(tobs).any()
    total = {}
    for case in range(len(llm.CASES)):
        for k, v in models(300, case).stats.items():
            total[k] = total.get(k, 0) + v
    # each branch of step 3, p == 0, d <= 0, a NaN term, both clamps
    for key in ('nonpos_n0', 'nonpos_hit', 'n0', 'poisson', 'hit', 'p_zero', 'timed', 'd_nonpos', 'nan_tobs', 'nan',
                'clamp_hi', 'clamp_lo', 'first_bin', 'last_bin', 'just_below', 'just_above', 'no_bin'):
        assert total.get(key, 0) > 0, key
    zero_floor = models(300, 4).stats                           # floor == 0: m == 0 with n == 0 and with n > 0
    assert zero_floor['nonpos_n0'] > 0 and zero_floor['nonpos_hit'] > 0 and zero_floor['d_nonpos'] > 0
    assert models(300, 6).stats['p_zero'] > 0 and models(300, 7).stats['nan'] > 0
    assert (models(300, 7).bad > 0).all() and not models(300, 0).bad.any()
    two = models(2, 1).stats
    assert two['first_bin'] > 0 and two['just_above'] > 0, 'the bin edges on the 2-channel library'
    assert len({int(w) for w in models(300, 1).words}) > 6, 'the hypotheses differ'


def test_mu_is_the_expected_value(models, entries):
    """The mu inside the model is numpy_expect's, word for word; and with mode 0, no tobs
    and one hypothesis, ll is the integer sum of the per-channel words of
    chr_library_expect_host's mu."""
    from chroma.library import LibraryEntries
    for nchannels in (2, 300):
        made = lm.made_library(nchannels)
        want = lm.numpy_expect(made, entries)
        assert np.array_equal(models(nchannels, 0).mu.view(np.uint32), want.mu.view(np.uint32))
        lib = lm.host_library(made)
        nobs, _ = llm.made_observed(nchannels)
        mode, _, floor, tfloor = llm.CASES[0]
        for h in range(entries.nevents):
            first, last = int(entries.offsets[h]), int(entries.offsets[h + 1])
            one = LibraryEntries([0, last - first], entries.source[first:last], entries.nphotons[first:last],
                                 entries.t[first:last])
            mu = lib.expect(one).get().mu[0]
            q, bad = llm.term_words(mu, np.zeros(nchannels, np.float32), nobs, None, mode, floor, tfloor, made.inv)
            got = lib.log_likelihood(one, nobs, None, floor=floor).get()
            assert got.words[0] == q.sum() and got.bad[0] == bad


def test_gibbs_inequality():
    """A library of integer weights (emitted == 1) and a hypothesis A whose m equals nobs on
    every channel: A's word is strictly the largest of 33.  The margin to the runner-up is
    checked on the model to be far above the 2^-20 per channel the words resolve."""
    from types import SimpleNamespace
    from chroma.library import LibraryEntries
    r = np.random.RandomState(3)
    ns, nch = 8, 64
    counts = r.randint(1, 20, (ns, nch)).astype(np.uint32)
    made = SimpleNamespace(nsources=ns, nchannels=nch, tbins=0, t_lo=np.float32(0), inv=np.float32(0),
                           emitted=np.ones(ns, np.uint64), counts=counts.reshape(-1).copy(), tmin=None, thist=None)
    a_source, a_photons = 3, 5
    nobs = counts[a_source] * np.uint32(a_photons)
    others = [(s, n) for s in range(ns) for n in (3, 4, 5, 6, 7) if (s, n) != (a_source, a_photons)][:32]
    hyp = [(a_source, a_photons)] + others
    en = LibraryEntries(np.arange(len(hyp) + 1), [s for s, _ in hyp], [n for _, n in hyp], np.zeros(len(hyp)))
    want = llm.numpy_loglike(made, en, nobs, None, llm.POISSON, np.float32(0), np.float32(0))
    assert np.array_equal(want.mu[0], nobs.astype(np.float32))
    margin = (want.words[0] - want.words[1:].max()) / 2.0 ** 20
    print('margin to the runner-up: %.3f' % margin)
    assert margin > 1.0, 'far above nch * 2^-20 = %.1e' % (nch * 2.0 ** -20)
    got = lm.host_library(made).log_likelihood(en, nobs, None, floor=0.0).get()
    assert np.array_equal(got.words, want.words) and not got.bad.any()
    assert (got.words[0] > got.words[1:]).all()


# ------------------------------------------------------------------ the Python layer
def test_channels_conversion():
    from chroma import event
    from chroma.likelihood import LibraryLikelihood
    hit = np.array([True, False, True, True, False])
    t = np.array([3.0, 1e9, -2.0, 7.5, 4.0], np.float32)
    q = np.array([2.5, 0.4, -3.0, 1.49, np.nan], np.float32)
    ch = event.Channels(hit, t, q)
    n, tt = LibraryLikelihood.observed(ch, 'hit')
    assert n.dtype == np.uint32 and n.tolist() == [1, 0, 1, 1, 0]
    assert tt.dtype == np.float32 and tt[[0, 2, 3]].tolist() == [3.0, -2.0, 7.5] and np.isnan(tt[[1, 4]]).all()
    n, tt = LibraryLikelihood.observed(ch, 'poisson')
    assert n.tolist() == [2, 0, 0, 1, 0], 'rint(q), negatives and NaN to 0'
    assert np.isnan(tt[[1, 4]]).all() and tt[2] == -2.0, 't only at the hit channels'
    pair = (np.arange(5, dtype=np.uint32), None)
    assert LibraryLikelihood.observed(pair)[0] is pair[0]


def test_library_likelihood_on_the_host_twin():
    """eval / scan / best through HostPhotonLibrary against the model."""
    from chroma import event
    from chroma.library import LibraryEntries, VoxelGrid
    from chroma.likelihood import LibraryLikelihood
    made = lm.made_library(300)
    grid = VoxelGrid((0, 0, 0), (4, 2, 1), (4, 2, 1))
    from chroma import gpu
    lib = gpu.HostPhotonLibrary(made, grid=grid)
    en = lm.made_entries()
    nobs, tobs = llm.made_observed(300)
    nobs = np.minimum(nobs, 50)
    ch = event.Channels(nobs > 0, np.where(nobs > 0, tobs, np.float32(1e9)).astype(np.float32), nobs.astype(np.float32))
    floor = np.float32(1e-3)
    tfl = llm.default_tfloor(made, floor)
    assert tfl == lib.default_tfloor(floor)
    for mode, code in (('poisson', llm.POISSON), ('hit', llm.HIT)):
        for use_times in (True, False):
            lik = LibraryLikelihood(lib, ch, mode=mode, floor=floor, use_times=use_times)
            n, t = LibraryLikelihood.observed(ch, mode)
            want = llm.numpy_loglike(made, en, n, t if use_times else None, code, floor, tfl if use_times else 0.0)
            got = lik.eval(en)
            assert got.dtype == np.float64 and np.array_equal(got, -(want.words / 2.0 ** 20))
            assert np.array_equal(lik.last.words, want.words) and lik.last.skipped == want.skipped
    # scan: one hypothesis per source, shaped to the grid
    lik = LibraryLikelihood(lib, ch, floor=floor)
    n, t = LibraryLikelihood.observed(ch)
    ns = lm.NSOURCES
    single = lambda nph, t0: LibraryEntries(np.arange(ns + 1), np.arange(ns), np.full(ns, nph), np.full(ns, t0))      # noqa: E731
    want = -(llm.numpy_loglike(made, single(40, 1.5), n, t, llm.POISSON, floor, tfl).words / 2.0 ** 20)
    got = lik.scan(40, t0=1.5)
    assert got.shape == (4, 2, 1) and np.array_equal(got[:, :, 0], want.reshape(2, 4).T)
    assert got[1, 1, 0] == want[1 + 4 * 1]
    assert LibraryLikelihood(lm.host_library(made), ch, floor=floor).scan(40, t0=1.5).shape == (ns,)
    # best over a 2 x 2 product, split into more than one group
    table = {(nph, t0): -(llm.numpy_loglike(made, single(nph, t0), n, t, llm.POISSON, floor, tfl).words / 2.0 ** 20)
             for nph in (40, 400) for t0 in (0.0, 1.5)}
    (nph, t0), s = min(((k, int(np.argmin(v))) for k, v in table.items()), key=lambda kv: table[kv[0]][kv[1]])
    calls = []
    lik.group_bytes = 20 * 5                                    # five hypotheses per call: 32 in seven groups
    inner = lib.log_likelihood
    lib.log_likelihood = lambda entries, *a, **k: calls.append(entries.nevents) or inner(entries, *a, **k)
    assert lik.best((40, 400), (0.0, 1.5)) == (s, nph, t0, float(table[(nph, t0)][s]))
    assert calls == [5] * 6 + [2]


def test_best_splits_at_what_one_call_accepts():
    """A product of more hypotheses than one call accepts (hypotheses x nchannels <= 2^31,
    the limit inherited from expect): best() splits there, although group_bytes would allow
    more, and every group is one the library accepts.  The calls are checked and counted,
    not computed: 720,000 hypotheses on 4097 channels would take the host twin minutes."""
    from types import SimpleNamespace
    from chroma.library import MAX_WORDS, LibraryEntries
    from chroma.likelihood import LibraryLikelihood
    lib = lm.host_library(lm.made_library(4097))
    cap = MAX_WORDS // 4097
    nph, t0 = np.arange(1, 301), np.arange(300)
    total = len(nph) * len(t0) * lm.NSOURCES
    assert cap < total < LibraryLikelihood.group_bytes // 20, 'the byte budget alone would send one call'
    with pytest.raises(ValueError, match='exceed 2\\^31'):      # refused before any work is done
        lib.log_likelihood(LibraryEntries(np.arange(total + 1), np.zeros(total), np.ones(total), np.zeros(total)),
                           np.zeros(4097, np.uint32))
    sizes = []

    def counted(entries, *args, **kwargs):
        lib._entries(entries)                                   # the refusal a real call makes
        sizes.append(entries.nevents)
        ll = -(entries.nphotons.astype(np.float64) + entries.t + entries.source / 16.0)
        return SimpleNamespace(get=lambda: SimpleNamespace(ll=ll))
    lik = LibraryLikelihood(lib, (np.zeros(4097, np.uint32), None))
    lib.log_likelihood = counted
    assert lik.best(nph, t0) == (0, 1, 0.0, 1.0), 'the minimum of the made values, found across the groups'
    assert sizes == [cap, total - cap] and max(sizes) * 4097 <= MAX_WORDS
    sizes.clear()
    lik.group_bytes = 20 * 10000                                # the byte budget, where it is the smaller one
    lik.best(nph[:50], t0[:50])
    assert sizes == [10000] * 2


def test_log_likelihood_refuses_in_python():
    lib = lm.host_library(lm.made_library(2))
    en = lm.made_entries()
    n = np.zeros(2, np.uint32)
    with pytest.raises(ValueError):
        lib.log_likelihood(en, n, mode='gauss')
    with pytest.raises(ValueError):
        lib.log_likelihood(en, np.zeros(3, np.uint32))
    with pytest.raises(ValueError):
        lib.log_likelihood(en, np.array([-1, 0]))
    with pytest.raises(ValueError):
        lib.log_likelihood(en, n, floor=-1.0)
    with pytest.raises(ValueError):
        lm.host_library(lm.made_library(2, thist=False)).log_likelihood(en, n, np.zeros(2, np.float32))
    with pytest.raises(TypeError):
        lib.log_likelihood(([0], [], [], []), n)
    none = lib.log_likelihood(type(en)([0], [], [], []), n).get()
    assert none.words.shape == (0,) and none.skipped == 0


# ------------------------------------------------------------------ the host twin in a stand-alone program
def test_stand_alone_host_program(tmp_path):
    """tests/library_loglike_host_check.cpp with csrc/library_host.cpp, built for the host:
    the twin and its refusals over heap blocks of exactly the documented sizes (the program
    a sanitizer build checks; here it is built plain)."""
    from test_host_driver import CSRC, ROOT, _compiler
    exe = str(tmp_path / 'library_loglike_host_check')
    subprocess.check_call([_compiler(), '-O2', '-std=c++17', '-Wall', '-ffp-contract=off', '-I', CSRC, '-o', exe,
                           os.path.join(ROOT, 'tests', 'library_loglike_host_check.cpp'),
                           os.path.join(CSRC, 'library_host.cpp'), '-lm'])
    p = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, timeout=120)
    print(p.stdout)
    assert p.stdout.strip().splitlines()[-1] == 'variants=4 failures=0' and p.returncode == 0
