#!/usr/bin/env python3
"""Dev tool (GPU box): time the photon-library log-likelihood (chr_library_loglike through
GPUPhotonLibrary's arrays) against the route a user has without it.  Prints one JSON line
per case; the records are kept under profiles/library_loglike/.

For every channel count of --channels (29007 = the benchmark detector's PMTs) and every
source count of --sources, a made library (counts, and a time histogram of --tbins bins)
and one observed event, scored against two tables of hypotheses:
  table   --hypotheses hypotheses of --entries entries on random sources;
  scan    one hypothesis per source with one entry: the full vertex scan.
Timed on each:
  loglike          chr_library_loglike, Poisson without times, on every path the shape admits;
  loglike_timed    the same with observed times (the histogram gather);
  expect           chr_library_expect alone on the same table (mu only: the library is given
                   without tmin), the kernel whose structure loglike inherits;
  expect_torch_f32 / _f64
                   the baseline: chr_library_expect, then sum over channels of
                   n * log(mu + floor) - mu with torch on the device in float32 / float64 (its
                   result agrees with the words to rounding, not bit for bit).  There is no
                   such route for the time term: expect gives no time density.

Device times are HIP events around one call, after a warm-up, over --repeats repeats; the
median, minimum and maximum are reported.  `bytes` is what the kernel must read: entries x
nchannels x 4 B of counts rows, the observed words, and for loglike_timed one 4-byte
histogram word per (entry, hit channel whose time falls into a bin) at most -- each of
which costs the memory system a whole line; `hbm_fraction` is bytes / time / 8 TB/s.

usage: tools/library_loglike_timing.py [--channels 29007,300] [--sources 1000,4000] [--hypotheses 64]
                                       [--entries 256] [--tbins 16] [--repeats 20]"""
import argparse
import ctypes
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))
sys.path.insert(0, ROOT)

from library_timing import HBM_BYTES_PER_S, summary, timed  # noqa: E402  (tools/: the same clock for both tools)

FLOOR = 1e-3


def case(args, nch, ns):
    import torch
    from chroma import gpu
    from chroma.gpu import _native, gpuarray as ga
    from chroma.gpu.tools import current_stream
    from chroma.library import LibraryEntries
    r = np.random.RandomState(7)
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    tb = args.tbins
    counts = ga.from_tensor(torch.randint(0, 30, (ns * nch,), dtype=torch.int32, device=dev, generator=g), np.uint32)
    thist = ga.from_tensor(torch.randint(0, 6, (ns * nch * tb,), dtype=torch.int32, device=dev, generator=g),
                           np.uint32)
    t_lo, inv = np.float32(0.0), np.float32(tb) / np.float32(200.0)
    emitted = ga.to_gpu(np.full(ns, 100000, np.uint64))
    lib = gpu.GPUPhotonLibrary(SimpleNamespace(nsources=ns, nchannels=nch, tbins=tb, t_lo=t_lo, inv=inv,
                                               emitted=emitted, counts=counts, tmin=None, thist=thist))
    # expect's library: the same counts, no histogram
    plain = gpu.GPUPhotonLibrary(SimpleNamespace(nsources=ns, nchannels=nch, tbins=0, t_lo=np.float32(0),
                                                 inv=np.float32(0), emitted=emitted, counts=counts, tmin=None,
                                                 thist=None))
    nobs = r.poisson(0.7, nch).astype(np.uint32)
    tobs = r.uniform(0.0, 220.0, nch).astype(np.float32)
    d_n, d_t = ga.to_gpu(nobs), ga.to_gpu(tobs)
    nhit = int((nobs > 0).sum())
    nev, per = args.hypotheses, args.entries
    tables = {'table': LibraryEntries(np.arange(nev + 1) * per, r.randint(0, ns, nev * per),
                                      r.randint(1, 5000, nev * per), r.uniform(0.0, 10.0, nev * per)),
              'scan': LibraryEntries(np.arange(ns + 1), np.arange(ns), np.full(ns, 2000), np.zeros(ns))}
    for name, en in tables.items():
        keep, desc = lib._upload_entries(en)
        nhyp, nent = en.nevents, en.nentries
        ll, bad = ga.empty(nhyp, np.int64), ga.empty(nhyp, np.uint32)
        mu = ga.empty(nhyp * nch, np.float32)
        skipped = ga.zeros(1, np.uint64)
        base = dict(nchannels=nch, sources=ns, shape=name, hypotheses=nhyp, entries=nent, hit_channels=nhit)
        row_bytes = nent * nch * 4
        _, plain_obs = lib._observed(d_n, None, 'poisson', FLOOR, None)
        _, timed_obs = lib._observed(d_n, d_t, 'poisson', FLOOR, None)

        def loglike(obs):
            return lambda: _native.call('chr_library_loglike', ctypes.byref(lib._desc()), ctypes.byref(desc),
                                        ctypes.byref(obs), ll.gpudata, bad.gpudata, skipped.gpudata, current_stream())

        def expect():
            _native.call('chr_library_expect', ctypes.byref(plain._desc()), ctypes.byref(desc), mu.gpudata, None,
                         skipped.gpudata, current_stream())

        n_f = {torch.float32: d_n.tensor.to(torch.float32), torch.float64: d_n.tensor.to(torch.float64)}

        def expect_torch(dtype):
            def route():
                expect()
                m = mu.tensor.view(nhyp, nch).to(dtype) + FLOOR
                return (n_f[dtype] * torch.log(m) - m).sum(dim=1)
            return route

        med = {}
        words = {}
        for what, obs, nbytes in (('loglike', plain_obs, row_bytes + nch * 4),
                                  ('loglike_timed', timed_obs, row_bytes + nch * 8 + nent * nhit * 4)):
            # forced narrow only where a wide path exists: without times, nchannels a multiple of 4
            for forced in ((None, 'n') if nch % 4 == 0 and what == 'loglike' else (None,)):
                if forced:
                    os.environ['CHR_LIBRARY_PATH'] = forced
                ms = timed(loglike(obs), args.repeats)
                os.environ.pop('CHR_LIBRARY_PATH', None)
                path = 'wide' if _native.lib().chr_library_loglike_last_path() == 1 else 'narrow'
                m = float(np.median(ms))
                med[what] = min(m, med.get(what, m))
                words[what] = ll.get()
                print(json.dumps(dict(base, what=what, path=path, per_call=summary(ms), bytes=nbytes,
                                      gbytes_per_s=round(nbytes / m / 1e6, 1),
                                      hbm_fraction=round(nbytes / (m * 1e-3) / HBM_BYTES_PER_S, 4),
                                      bad=int(bad.get().sum()))), flush=True)
        ms = timed(expect, args.repeats)
        med['expect'] = float(np.median(ms))
        print(json.dumps(dict(base, what='expect', per_call=summary(ms), bytes=row_bytes,
                              gbytes_per_s=round(row_bytes / med['expect'] / 1e6, 1),
                              loglike_over_expect=round(med['loglike'] / med['expect'], 3),
                              loglike_timed_over_expect=round(med['loglike_timed'] / med['expect'], 3))), flush=True)
        ours = words['loglike'].astype(np.float64) / 2.0 ** 20
        for dtype, label in ((torch.float32, 'expect_torch_f32'), (torch.float64, 'expect_torch_f64')):
            ms = timed(expect_torch(dtype), args.repeats)
            theirs = expect_torch(dtype)().cpu().numpy().astype(np.float64)
            m = float(np.median(ms))
            print(json.dumps(dict(base, what=label, per_call=summary(ms),
                                  max_rel_diff_to_loglike=float(np.max(np.abs(theirs - ours) / np.abs(ours))),
                                  over_loglike=round(m / med['loglike'], 2),
                                  over_loglike_timed=round(m / med['loglike_timed'], 2))), flush=True)
        del keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--channels', default='29007,300')
    ap.add_argument('--sources', default='1000,4000')
    ap.add_argument('--hypotheses', type=int, default=64)
    ap.add_argument('--entries', type=int, default=256)
    ap.add_argument('--tbins', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=20)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'library_loglike_timing needs a HIP device'
    torch.cuda.set_device(0)
    from chroma.gpu import create_cuda_context
    create_cuda_context()
    print(json.dumps(dict(what='setup', device=torch.cuda.get_device_name(0), tbins=args.tbins, floor=FLOOR,
                          repeats=args.repeats)), flush=True)
    for nch in [int(x) for x in args.channels.split(',')]:
        for ns in [int(x) for x in args.sources.split(',')]:
            case(args, nch, ns)
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
