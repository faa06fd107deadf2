"""Child process of tests/test_gpu_photon_tracks.py: an untracked propagate on
the 2-PMT detector in a process that never made a tracked call, for the test's
comparison with untracked runs made before and after a tracked one.  The run
itself is untracked_run(), which the test calls too.
usage: photon_tracks_child.py OUT.npz"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))

import numpy as np  # noqa: E402

N, SEED, NTPB, MAX_BLOCKS, MAX_STEPS = 12000, 61, 64, 128, 30     # cap 8192: steps above and below the tail threshold
FIELDS = ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx')


def untracked_run(gg):
    """{field: uint32 words} of the photons and 'rng' after propagate(track=False)."""
    from chroma import gpu
    from chroma.photon_source import isotropic
    rng = gpu.get_rng_states(NTPB * MAX_BLOCKS, seed=SEED)
    gp = gpu.GPUPhotons(isotropic(N, seed=SEED))
    gp.propagate(gg, rng, nthreads_per_block=NTPB, max_blocks=MAX_BLOCKS, max_steps=MAX_STEPS)
    got = gp.get()
    out = {f: np.ascontiguousarray(getattr(got, f)).view(np.uint32) for f in FIELDS}
    out['rng'] = rng.get().reshape(-1)
    return out


def main(out):
    import torch
    from chroma import demo, gpu, loader
    torch.cuda.set_device(0)
    geo = loader.create_geometry_from_obj(demo.detector(600.0, 900.0, 1500.0))
    np.savez(out, **untracked_run(gpu.GPUGeometry(geo)))


if __name__ == '__main__':
    main(sys.argv[1])
