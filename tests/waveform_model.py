"""What the waveform tests share: a numpy restatement of the DAQ's draws per
photon (the photoelectron records of chr_daq_acquire_events_pe), of the charge
trains and of the digitiser (include/chroma_amd.h, "waveforms") -- the expected
words never come from the code under test.  The draws take their uniforms from
the oracle's generator (oracle.uniforms) and restate the rest in float32: the
acceptance, daq.hip's interp in its operation order, the rounding of the charge.
test_waveforms.py anchors the records: folded per (event, channel) they must
give oracle_events' channel words and RNG states."""
import math

import numpy as np

import oracle
from library_model import fmaf, sat_u32

f32, u32 = np.float32, np.uint32
NO_HIT_TIME = f32(1e9)
NO_HIT_BITS = NO_HIT_TIME.view(u32)
SURFACE_DETECT = 0x4


# ---------------------------------------------------------------- the draws
def interp(x, xp, fp):
    """daq.hip's interp (interpolate.h:32-58) in float32, the same operations in the same order."""
    lower, upper = 0, len(xp) - 1
    if x <= xp[lower]:
        return fp[lower]
    if x >= xp[upper]:
        return fp[upper]
    while lower < upper - 1:
        half = (lower + upper) // 2
        if x < xp[half]:
            upper = half
        else:
            lower = half
    df = f32(fp[upper] - fp[lower])
    dx = f32(xp[upper] - xp[lower])
    return f32(fp[lower] + f32(f32(df * f32(x - xp[lower])) / dx))


def roundf(x):
    """C's roundf of a float32: halfway cases away from zero (exact in float64)."""
    x = float(x)
    if not math.isfinite(x):
        return f32(x)
    return f32(math.copysign(math.floor(abs(x) + 0.5), x))


def candidate_channels(detector, photons):
    """candidate_channel (daq.hip) of every photon: its channel where the DAQ draws for it, else -1."""
    solid = np.asarray(detector.solid_id)
    s2c = np.asarray(detector.solid_id_to_channel_index)
    nch = int(detector.num_channels())
    tri = np.asarray(photons.last_hit_triangles)
    ok = (tri > -1) & ((np.asarray(photons.flags) & SURFACE_DETECT) != 0)
    c = np.full(len(tri), -1, np.int32)
    c[ok] = s2c[solid[tri[ok]]]
    c[(c < 0) | (c >= nch)] = -1
    return c


def records(detector, photons, states, nslots, bounds, ntpb, max_blocks, weight=1.0):
    """The photoelectron records of the events [bounds[e], bounds[e+1]): (pe_channel,
    pe_time, pe_q) over the span, indexed from bounds[0].  `states` (the oracle's
    6*nslots words) is advanced in place by exactly the uniforms the DAQ takes:
    slot s < min(cap, n_e) visits positions s, s + cap, ... of event e, events
    ascending; one uniform per candidate photon, two more when it is below
    weights * global_weight."""
    from chroma.gpu.detector import cdf_arrays
    tx, ty = cdf_arrays(detector.time_cdf)
    qx, qy = cdf_arrays(detector.charge_cdf)
    unit = f32(detector.charge_cdf[0][-1] / 2 ** 16)
    cand = candidate_channels(detector, photons)
    t = np.asarray(photons.t, f32)
    w = np.asarray(photons.weights, f32)
    bounds = np.asarray(bounds, np.int64)
    first, span = int(bounds[0]), int(bounds[-1] - bounds[0])
    cap = int(ntpb) * int(max_blocks)
    pe_c = np.full(span, -1, np.int32)
    pe_t = np.full(span, NO_HIT_TIME, f32)
    pe_q = np.zeros(span, u32)
    # the candidate photons of every slot, in the order the slot meets them
    per_slot = {}
    for b0, b1 in zip(bounds[:-1], bounds[1:]):
        n = int(b1 - b0)
        for pos in np.flatnonzero(cand[b0:b1] >= 0):
            per_slot.setdefault(int(pos) % cap, []).append(int(b0) + int(pos))
    # positions are met in ascending order within a slot and event: flatnonzero ascends
    for slot, mine in sorted(per_slot.items()):
        scratch = states.copy()
        u = oracle.uniforms(scratch, nslots, slot, 3 * len(mine))
        k = 0
        for p in mine:
            accept = u[k] < f32(w[p] * f32(weight))
            k += 1
            if not accept:
                continue
            time = f32(t[p] + interp(u[k], ty, tx))
            charge = interp(u[k + 1], qy, qx)
            k += 2
            pe_c[p - first] = cand[p]
            pe_t[p - first] = time
            with np.errstate(all='ignore'):
                pe_q[p - first] = sat_u32(roundf(f32(charge / unit)))[0]
        oracle.uniforms(states, nslots, slot, k)        # advance the real state by what was taken
    return pe_c, pe_t, pe_q


def event_of(bounds, span):
    """The event of every span position."""
    bounds = np.asarray(bounds, np.int64)
    return np.searchsorted(bounds, bounds[0] + np.arange(span), side='right') - 1


def fold(pe_c, pe_t, pe_q, flags, bounds, nchannels):
    """The channel rows the records fold to: unsigned minimum of the time bit
    patterns, charge sum mod 2^32, OR of the accepted photons' histories."""
    nevents = len(bounds) - 1
    t = np.full((nevents, nchannels), NO_HIT_BITS, u32)
    q = np.zeros((nevents, nchannels), u32)
    fl = np.zeros((nevents, nchannels), u32)
    ev = event_of(bounds, len(pe_c))
    hist = np.asarray(flags, u32)[int(bounds[0]):int(bounds[0]) + len(pe_c)]
    kept = np.flatnonzero(pe_c >= 0)
    np.minimum.at(t, (ev[kept], pe_c[kept]), pe_t[kept].view(u32))
    np.add.at(q, (ev[kept], pe_c[kept]), pe_q[kept])
    np.bitwise_or.at(fl, (ev[kept], pe_c[kept]), hist[kept])
    return t, q, fl


# ---------------------------------------------------------------- the trains
def hit_map_of(time_words):
    """row_of_word of the zero-suppressed read-out, and its row count."""
    hit = np.asarray(time_words, u32).reshape(-1) != NO_HIT_BITS
    return np.where(hit, np.cumsum(hit) - 1, -1).astype(np.int32), int(hit.sum())


def trains(pe_c, pe_t, pe_q, bounds, nchannels, row_of_word, nrows, t_lo, inv, nsamples):
    """(trains (nrows, nsamples), outside_q, dropped): float32 subtract, then multiply, then the two comparisons."""
    out = np.zeros((nrows, nsamples), u32)
    outside = np.zeros(nrows, u32)
    kept = np.flatnonzero(pe_c >= 0)
    word = event_of(bounds, len(pe_c))[kept] * nchannels + pe_c[kept]
    row = word if row_of_word is None else np.asarray(row_of_word)[word]
    has_row = (row >= 0) & (row < nrows)
    dropped = int((~has_row).sum())
    kept, row = kept[has_row], row[has_row]
    with np.errstate(all='ignore'):
        d = (pe_t[kept] - f32(t_lo)).astype(f32)
        x = (d * f32(inv)).astype(f32)
        inside = (x >= f32(0.0)) & (x < f32(nsamples))
        b = np.where(inside, x, 0).astype(np.int64)
    np.add.at(out, (row[inside], b[inside]), pe_q[kept][inside])
    np.add.at(outside, row[~inside], pe_q[kept][~inside])
    return out, outside, dropped


# ---------------------------------------------------------------- the digitiser
def digitise(train_rows, template, scale, pedestal, adc_max):
    """(adc (nrows, nsamples) uint16, bad): taps ascending, single-rounded multiply-adds."""
    train_rows = np.asarray(train_rows, u32)
    nrows, nsamples = train_rows.shape
    taps = np.asarray(template, f32)
    charge = train_rows.astype(f32)
    v = np.zeros((nrows, nsamples), f32)
    for k in range(min(len(taps), nsamples)):
        v[:, k:] = fmaf(taps[k], charge[:, :nsamples - k], v[:, k:])
    v[~train_rows.any(axis=1)] = 0.0              # an empty row skips the convolution
    x = fmaf(v, f32(scale), f32(pedestal))
    nan = np.isnan(x)
    with np.errstate(all='ignore'):
        a = np.minimum(sat_u32((x + f32(0.5)).astype(f32).reshape(-1)), u32(adc_max)).reshape(x.shape)
    a[nan] = 0
    return a.astype(np.uint16), int(nan.sum())


# ---------------------------------------------------------------- the made case, computed once
_CASES = {}


def made_case(detector, ntpb, max_blocks, weight, nslots=64 * 1024, seed=5):
    """The made records of test_gpu_daq in the events of test_daq_events.BOUNDS on
    `detector` (its DAQ CDFs set by the caller): the oracle's channel words and
    final RNG states, and the model's records with the states they leave.  One
    computation per parameter set and session; callers must not write to it."""
    from types import SimpleNamespace
    from test_daq_events import BOUNDS, oracle_events
    from test_gpu_daq import _made_records
    key = (int(ntpb), int(max_blocks), float(weight), int(nslots), int(seed))
    if key not in _CASES:
        photons, kind = _made_records(detector)
        host = oracle.HostPhotons(photons)
        st = oracle.rng_init(nslots, seed=seed)
        t, q, fl, _ = oracle_events(detector, host, st, nslots, BOUNDS, ntpb, max_blocks, weight)
        model_st = oracle.rng_init(nslots, seed=seed)
        pe = records(detector, photons, model_st, nslots, BOUNDS, ntpb, max_blocks, weight)
        case = SimpleNamespace(photons=photons, kind=kind, bounds=BOUNDS, nslots=nslots, seed=seed,
                               nchannels=int(detector.num_channels()), t=t, q=q, fl=fl, states=st,
                               pe=pe, model_states=model_st,
                               unit=f32(detector.charge_cdf[0][-1] / 2 ** 16))
        for a in (t, q, fl, st, model_st) + pe:
            a.setflags(write=False)
        _CASES[key] = case
    return _CASES[key]
