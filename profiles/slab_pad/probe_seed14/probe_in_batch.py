# Dev probe (GPU box): the seed-14 photon of DESIGN 14.4; prints one JSON object.  CHROMA_AMD_LIB selects the library.
import json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'chroma-lite_amd'), os.path.join(ROOT, 'oracle')]
import numpy as np
import torch
import bench, oracle
from chroma import gpu
from chroma.photon_source import isotropic
from chroma.gpu.packing import PackedGeometry
torch.cuda.set_device(0)
geo = bench.build_geometry('29k', os.environ.get('CHROMA_BENCH_CACHE', '/tmp/chroma_bench_cache'))
packed = PackedGeometry(geo)
ph = isotropic(10_000_000, seed=14)
I = 1889288
out = {}
d = ph.dir[I:I + 1].astype(np.float32); o = ph.pos[I:I + 1].astype(np.float32)
n2 = np.float32(d[0, 0] * d[0, 0]) ; n2 = np.float32(n2 + np.float32(d[0, 1] * d[0, 1])); n2 = np.float32(n2 + np.float32(d[0, 2] * d[0, 2]))
dn = (d / np.sqrt(n2, dtype=np.float32)).astype(np.float32)
out['d'] = [float(x).hex() for x in d[0]]; out['dn'] = [float(x).hex() for x in dn[0]]
for name, dd in (('d', d), ('dn', dn)):
    for last in (-1, 93882364, 93886144):
        dist, tri = oracle.intersect_rays(packed, o, dd, np.array([last], np.int32))
        out['oracle_%s_excl_%d' % (name, last)] = [int(tri[0]), float(dist[0])]
lo_i = I - (1 << 16); k = I - lo_i
sub = ph[lo_i:lo_i + (1 << 17)]
out['sub_dir_same'] = bool(np.array_equal(sub.dir[k], ph.dir[I]))
NTPB, MAXB = 512, 1024
oracle.undershoot()
host = oracle.HostPhotons(sub); host.last_hit_triangles[:] = -1; host.weights[:] = 1.0
oracle.propagate(packed, host, oracle.rng_init(NTPB * MAXB, seed=1), NTPB * MAXB, NTPB, MAXB, 1)
out['oracle_undershoot_sub'] = oracle.undershoot()
out['oracle_in_batch'] = dict(tri=int(host.last_hit_triangles[k]), flags=int(host.flags[k]), pos=host.pos[k].tolist(),
                              r=float(np.linalg.norm(host.pos[k].astype(np.float64))), t=float(host.t[k]))
gdet = gpu.GPUDetector(geo)
res = []
for rep in range(12):
    gp = gpu.GPUPhotons(sub, copy_flags=True, copy_triangles=False, copy_weights=False)
    rng = gpu.get_rng_states(NTPB * MAXB, seed=1)
    gp.propagate(gdet, rng, nthreads_per_block=NTPB, max_blocks=MAXB, max_steps=1)
    g = gp.get()
    res.append(dict(tri=int(g.last_hit_triangles[k]), flags=int(g.flags[k]), r=float(np.linalg.norm(g.pos[k].astype(np.float64))),
                    mism=int((g.last_hit_triangles != host.last_hit_triangles).sum())))
out['gpu_in_batch'] = res
# the whole first batch of the sweep (5 M photons), one step, a few repeats: which triangle
big = ph[:5_000_000]
hb = oracle.HostPhotons(big); hb.last_hit_triangles[:] = -1; hb.weights[:] = 1.0
oracle.propagate(packed, hb, oracle.rng_init(NTPB * MAXB, seed=1), NTPB * MAXB, NTPB, MAXB, 1)
out['oracle_undershoot_5M'] = oracle.undershoot()
out['oracle_5M'] = dict(tri=int(hb.last_hit_triangles[I]), flags=int(hb.flags[I]), r=float(np.linalg.norm(hb.pos[I].astype(np.float64))))
res = []
for rep in range(8):
    gp = gpu.GPUPhotons(big, copy_flags=True, copy_triangles=False, copy_weights=False)
    rng = gpu.get_rng_states(NTPB * MAXB, seed=1)
    gp.propagate(gdet, rng, nthreads_per_block=NTPB, max_blocks=MAXB, max_steps=1)
    g = gp.get()
    res.append(dict(tri=int(g.last_hit_triangles[I]), r=float(np.linalg.norm(g.pos[I].astype(np.float64))),
                    mism=int((g.last_hit_triangles != hb.last_hit_triangles).sum())))
out['gpu_5M'] = res
print(json.dumps(out))
