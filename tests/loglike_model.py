"""What the photon-library log-likelihood tests share: a numpy restatement of the rule
(include/chroma_amd.h, "Log-likelihood") -- the expected words never come from the code
under test -- over library_model's float32 arithmetic (fmaf, logf, expf, not copied), the
made observed events and the cases the made records are run through."""
from types import SimpleNamespace

import numpy as np

import library_model as lm
from library_model import expf, fmaf, host_library, logf, made_entries, made_library  # noqa: F401  (shared with the tests)

f32, u32 = np.float32, np.uint32
LIMIT = f32(8388608.0)            # 2^23
SCALE = f32(1048576.0)            # 2^20
POISSON, HIT = 0, 1


def _logf(x):
    """chr_logf of positive float32 that are normal or +inf (log(+inf) = +inf)."""
    x = np.atleast_1d(np.asarray(x, f32))
    out = np.full(x.shape, np.inf, f32)
    finite = np.isfinite(x)
    if finite.any():
        out[finite] = logf(x[finite])
    return out


def _one_minus_exp(m):
    """1.0f - chr_expf(-m) for m > 0.  From m = 32 on the model takes 1.0f without
    evaluating chr_expf: its result there is at most e^-32 (1 + 2^-22) < 2^-45, far below
    half an ulp of 1.0f (2^-25), so the subtraction rounds to 1.0f whatever its last bits."""
    m = np.atleast_1d(np.asarray(m, f32))
    out = np.ones(m.shape, f32)
    small = m < f32(32.0)
    if small.any():
        out[small] = f32(1.0) - expf(-m[small])
    return out


def time_bin(t, t_lo, inv, ntbins):
    """The hit map's bin function (rule step 6 of a hit map): one float32 subtract, one
    float32 multiply; -1 where the time falls into no bin.  Returns (bin, x)."""
    with np.errstate(invalid='ignore', over='ignore'):
        x = (np.asarray(t, f32) - f32(t_lo)) * f32(inv)
        ok = (x >= 0) & (x < f32(ntbins))
    return np.where(ok, np.where(ok, x, 0).astype(np.int64), -1), x


def term_words(mu, a, n, tobs, mode, floor, tfloor, inv, stats=None):
    """Steps 2-5 for the channels of one hypothesis: (q as int64 per channel, bad)."""
    st = stats if stats is not None else {}
    count = lambda key, mask: st.__setitem__(key, st.get(key, 0) + int(np.count_nonzero(mask)))      # noqa: E731
    mu, a, n = np.asarray(mu, f32), np.asarray(a, f32), np.asarray(n, u32)
    with np.errstate(all='ignore'):
        m = mu + f32(floor)
        pos = m > 0
    term = np.zeros(len(m), f32)
    term[~pos & (n > 0)] = -LIMIT
    count('nonpos_n0', ~pos & (n == 0)), count('nonpos_hit', ~pos & (n > 0))
    dark = pos & (n == 0)
    term[dark] = -m[dark]
    count('n0', dark)
    lit = pos & (n > 0)
    if mode == POISSON:
        term[lit] = fmaf(n[lit].astype(f32), _logf(m[lit]), -m[lit])
        count('poisson', lit)
    else:
        p = _one_minus_exp(m[lit])
        lp = np.full(len(p), -LIMIT, f32)
        lp[p > 0] = _logf(p[p > 0])
        term[lit] = lp
        count('hit', p > 0), count('p_zero', ~(p > 0))
    if tobs is not None:
        timed = lit & ~np.isnan(tobs)
        d = fmaf(a[timed], f32(inv), f32(tfloor))
        ld = np.full(len(d), -LIMIT, f32)
        ld[d > 0] = _logf(d[d > 0])
        with np.errstate(invalid='ignore'):
            term[timed] = (term[timed] + ld) - _logf(m[timed])
        count('timed', d > 0), count('d_nonpos', ~(d > 0)), count('nan_tobs', lit & np.isnan(tobs))
    nan = np.isnan(term)
    count('nan', nan), count('clamp_hi', term > LIMIT), count('clamp_lo', term < -LIMIT)
    with np.errstate(invalid='ignore'):
        clamped = np.minimum(np.maximum(term, -LIMIT), LIMIT)
    q = np.zeros(len(m), np.int64)
    q[~nan] = np.trunc((clamped[~nan] * SCALE).astype(np.float64)).astype(np.int64)      # the product is exact in float32
    return q, int(nan.sum())


def numpy_loglike(lib, en, nobs, tobs=None, mode=POISSON, floor=f32(1e-3), tfloor=f32(0)):
    """words (int64), bad, skipped of the log-likelihood rule, with the mu it folded
    (nhypotheses, nchannels) and counts of what happened on the way (`stats`)."""
    nch, tb = lib.nchannels, lib.tbins
    n = np.asarray(nobs, u32)
    tobs = None if tobs is None else np.asarray(tobs, f32)
    words, bad = np.zeros(en.nevents, np.int64), np.zeros(en.nevents, u32)
    mus = np.zeros((en.nevents, nch), f32)
    stats = {}
    channel = np.arange(nch)
    for h in range(en.nevents):
        mu, a = np.zeros(nch, f32), np.zeros(nch, f32)
        for i in range(int(en.offsets[h]), int(en.offsets[h + 1])):
            s, w = lm._entry_of(lib, en, i)
            if s is None:
                continue
            mu = fmaf(w, lib.counts[s * nch:(s + 1) * nch].astype(f32), mu)
            if tobs is not None:
                with np.errstate(invalid='ignore'):
                    b, x = time_bin(tobs - f32(en.t[i]), lib.t_lo, lib.inv, tb)
                take = (n > 0) & (b >= 0)
                word = (s * nch + channel[take]) * tb + b[take]
                a[take] = fmaf(w, lib.thist[word].astype(f32), a[take])
                lit = n > 0
                for key, mask in (('first_bin', take & (b == 0)), ('last_bin', take & (b == tb - 1)),
                                  ('just_below', lit & (x < 0) & (x > -1e-3)),
                                  ('just_above', lit & (x >= tb) & (x < tb + 1e-3)),
                                  ('no_bin', lit & (b < 0))):
                    stats[key] = stats.get(key, 0) + int(mask.sum())
        mus[h] = mu
        q, nbad = term_words(mu, a, n, tobs, mode, floor, tfloor, lib.inv, stats)
        words[h], bad[h] = q.sum(), nbad
    sources = en.source[int(en.offsets[0]):int(en.offsets[-1])]
    return SimpleNamespace(words=words, bad=bad, skipped=int((sources >= lib.nsources).sum()), mu=mus, stats=stats)


# ---------------------------------------------------------------- the made observed events and cases
def made_observed(nchannels, seed=21):
    """nobs, tobs for a made library.  Channels 0 and 1 are the ones made_entries' 9-entry
    event aims at (entry times 1.0, 2.0, NaN, -3.0, 0.5, 4.0, -50.0, NaN on sources 0 and 1;
    the histogram covers [-8, 24) in four bins): nobs 2^24 + 1 and 3; tobs -7.0 (1.0 - 8.0: the
    first bin's lower edge) and 26.0 (2.0 + 24.0: the upper edge, just outside).  From 300
    channels on, channels 2 .. 10 hold: the time just below -7.0, just below 26.0 (the last
    bin), NaN, +inf, -inf, and counts of 2^24, 10^6 and 0 at a NaN time."""
    r = np.random.RandomState(seed + nchannels)
    nobs = r.randint(0, 5, nchannels).astype(u32)
    nobs[r.uniform(size=nchannels) < 0.4] = 0
    tobs = r.uniform(-20.0, 60.0, nchannels).astype(f32)
    tobs[r.uniform(size=nchannels) < 0.05] = np.nan
    nobs[0:2] = (2 ** 24 + 1, 3)
    tobs[0:2] = (-7.0, 26.0)
    if nchannels >= 11:
        nobs[2:11] = (1, 2, 1, 5, 1, 2 ** 24, 10 ** 6, 0, 7)
        tobs[2:11] = (-7.000002, 25.99999, np.nan, np.inf, -np.inf, 3.0, 4.0, np.nan, 2.5)
    return nobs, tobs


INF = f32(np.inf)
# (mode, with tobs, floor, tfloor; None: floor / (t_hi - t_lo)): both modes with and without times; floor 0,
# so that m == 0 meets n == 0 and n > 0, with tfloor 0, so that d == 0 where no bin is found; a floor so
# small that 1 - expf(-m) == 0 for the hypotheses without entries; an infinite floor, whose Poisson term
# fmaf(n, +inf, -inf) is a NaN
CASES = [(POISSON, False, f32(1e-3), f32(0)), (POISSON, True, f32(1e-3), None), (HIT, False, f32(1e-3), f32(0)),
         (HIT, True, f32(1e-3), None), (POISSON, True, f32(0), f32(0)), (HIT, True, f32(0), f32(0)),
         (HIT, False, f32(1e-9), f32(0)), (POISSON, False, INF, f32(0))]


def default_tfloor(lib, floor):
    """floor / (t_hi - t_lo) as the Python layer computes it: in float64 from inv = ntbins / (t_hi - t_lo)."""
    return f32(float(f32(floor)) * float(lib.inv) / lib.tbins)


def trailing_empty(en):
    """made_entries followed by a run of three hypotheses without entries."""
    from chroma.library import LibraryEntries
    return LibraryEntries(np.concatenate([en.offsets, [en.offsets[-1]] * 3]), en.source, en.nphotons, en.t)
