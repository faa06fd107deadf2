#!/usr/bin/env python3
"""Dev tool (GPU box): time chr_generate_photons against the parent's way of
getting the same photons onto the device.

  flash   10 M photons from one isotropic-flash genstep
  mixed   10 M photons from 10^4 gensteps of 1000 photons (Cherenkov,
          scintillation and isotropic in turn, along random segments), and
          the same steps all of one kind (steps_*)
  upload  photon_source.isotropic(10 M) drawn with numpy on the host, then
          GPUPhotons(...) (the 40 B/photon upload): what a caller did before

Geometry: chroma.demo.scint.tiny() (dispersive liquid scintillator with two
re-emission components); RNG: the simulation's 524,288 slots.  Generation is
timed with HIP events recorded before and after the call on its (idle) stream
(warm-up, then 20 repeats; median, min, max): the call's host work (resolving
materials, validation, staging the records), the record upload, the kernel and
the counter's download; and with a host clock around the same.  The kernel
alone is read from a rocprofv3 kernel trace of this tool (profiles/gensteps/).  The
bytes are the 40 B each photon's nine fields take; the peak is the MI355X's
8 TB/s HBM3E.  Prints one JSON line per case.

usage: tools/gensteps_timing.py [nphotons] [repeats] [upload_repeats]"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))

BYTES_PER_PHOTON = 40
PEAK_BYTES_PER_S = 8e12


def mixed_steps(material, nsteps, per_step, seed=1, kinds=(0, 1, 2)):
    from chroma import gensteps as gs
    rng = np.random.default_rng(seed)
    rec = np.zeros(nsteps, gs.GENSTEP_DTYPE)
    rec['kind'] = np.asarray(kinds, np.uint32)[np.arange(nsteps) % len(kinds)]   # the kinds in turn
    rec['nphotons'] = per_step
    rec['x0'] = rng.uniform(-500, 500, (nsteps, 3))
    d = rng.normal(size=(nsteps, 3))
    rec['dx'] = 10.0 * d / np.linalg.norm(d, axis=1)[:, None]
    rec['t0'] = rng.uniform(0, 10, nsteps)
    rec['dt'] = 0.03
    rec['wl_lo'], rec['wl_hi'] = 300.0, 600.0
    rec['beta'] = rng.uniform(0.9, 1.0, nsteps)
    rec['component'] = np.where(rec['kind'] == gs.SCINTILLATION, np.arange(nsteps) // 3 % 2, 0)
    return gs.Gensteps(rec, [material] * nsteps)


def summary(ms):
    ms = np.asarray(ms)
    return dict(median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4),
                max_ms=round(float(ms.max()), 4))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    upload_repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    os.environ.setdefault('CHROMA_CACHE_DIR', tempfile.mkdtemp(prefix='chroma_cache_timing_'))
    import torch
    from chroma import gensteps as gs
    from chroma import gpu, loader
    from chroma.demo import scint
    from chroma.gpu.photon import _alloc
    from chroma.photon_source import isotropic
    assert torch.cuda.is_available(), 'gensteps_timing needs a HIP device'
    torch.cuda.set_device(0)
    geo = loader.create_geometry_from_obj(scint.tiny())
    gg = gpu.GPUGeometry(geo)
    ls = [m for m in gg.packed.material_objects if m.name == 'liquid_scintillator'][0]
    nslots = 512 * 1024
    rng = gpu.get_rng_states(nslots, seed=1)
    per_step = 1000
    nsteps = max(1, n // per_step)
    cases = [('flash', gs.isotropic_flash(ls, n)), ('mixed', mixed_steps(ls, nsteps, per_step)),
             # the mixed case's steps, all of one kind: where its time goes
             ('steps_isotropic', mixed_steps(ls, nsteps, per_step, kinds=(gs.ISOTROPIC,))),
             ('steps_scintillation', mixed_steps(ls, nsteps, per_step, kinds=(gs.SCINTILLATION,))),
             ('steps_cherenkov', mixed_steps(ls, nsteps, per_step, kinds=(gs.CHERENKOV,)))]
    buf = type('H', (), _alloc(n))()
    for name, steps in cases:
        total = len(steps)
        for _ in range(3):
            made = gpu.generate_photons(steps, gg, rng, out=buf)
        ev_ms, wall_ms = [], []
        for _ in range(repeats):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            made = gpu.generate_photons(steps, gg, rng, out=buf)
            b.record()
            b.synchronize()
            wall_ms.append((time.perf_counter() - t0) * 1e3)
            ev_ms.append(a.elapsed_time(b))
        med = float(np.median(ev_ms))
        got = made.get()
        ok = bool(np.isfinite(got.dir).all() and np.abs(np.linalg.norm(got.dir.astype(np.float64), axis=1) - 1).max() < 1e-5)
        print(json.dumps(dict(case=name, photons=total, steps=steps.nsteps, rng_slots=nslots, exhausted=made.exhausted,
                              device=summary(ev_ms), host_call=summary(wall_ms),
                              photons_per_s=round(total / (med * 1e-3)),
                              write_GB_per_s=round(total * BYTES_PER_PHOTON / (med * 1e-3) / 1e9, 1),
                              share_of_peak_bandwidth=round(total * BYTES_PER_PHOTON / (med * 1e-3) / PEAK_BYTES_PER_S, 4),
                              unit_directions=ok)), flush=True)
    del buf, made
    draw_ms, up_ms = [], []
    for i in range(upload_repeats + 1 if upload_repeats else 0):
        t0 = time.perf_counter()
        ph = isotropic(n, seed=100 + i)
        t1 = time.perf_counter()
        gp = gpu.GPUPhotons(ph, copy_flags=True, copy_triangles=False, copy_weights=False)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i:                                            # the first pass warms the allocator
            draw_ms.append((t1 - t0) * 1e3)
            up_ms.append((t2 - t1) * 1e3)
        del gp, ph
    if upload_repeats:
        print(json.dumps(dict(case='upload', photons=n, host_draw=summary(draw_ms),
                              gpuphotons_upload=summary(up_ms),
                              total_median_ms=round(float(np.median(np.add(draw_ms, up_ms))), 2))), flush=True)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == '__main__':
    main()
