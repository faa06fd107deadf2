# Dev probe (GPU box): the seed-14 photon of DESIGN 14.4; prints one JSON object.  CHROMA_AMD_LIB selects the library.
import ctypes, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'chroma-lite_amd'), os.path.join(ROOT, 'oracle')]
import numpy as np
import torch
import bench, oracle
from chroma import gpu
from chroma.event import Photons
from chroma.photon_source import isotropic
from chroma.gpu import _native, gpuarray as ga
from chroma.gpu.packing import PackedGeometry
from chroma.gpu.tools import current_stream
torch.cuda.set_device(0)
geo = bench.build_geometry('29k', os.environ.get('CHROMA_BENCH_CACHE', '/tmp/chroma_bench_cache'))
packed = PackedGeometry(geo)
ph = isotropic(10_000_000, seed=14)
I = 1889288
o = np.array([ph.pos[I]], np.float32); d = np.array([ph.dir[I]], np.float32)
out = {'lib': os.environ.get('CHROMA_AMD_LIB', 'default'), 'o': o.tolist(), 'd': d.tolist(), 'o_hex': [float(x).hex() for x in o[0]], 'd_hex': [float(x).hex() for x in d[0]]}
dn = (d.astype(np.float32) / np.sqrt((d.astype(np.float32) ** 2).sum(dtype=np.float32))).astype(np.float32)
X, Y = 93882364, 93886144
dist, tri = oracle.intersect_rays(packed, o, d, np.array([-1], np.int32))
out['oracle'] = [int(tri[0]), float(dist[0])]
for name, last in (('excl_X', X), ('excl_Y', Y)):
    dist2, tri2 = oracle.intersect_rays(packed, o, d, np.array([last], np.int32))
    out['oracle_' + name] = [int(tri2[0]), float(dist2[0])]
# the two candidates: Moller-Trumbore in double and the reference leaf box entry
nodes = packed.nodes
leaf = (nodes[:, 3] >> 28) == 0
ids = (nodes[leaf, 3] & 0x0FFFFFFF)
wo, ws = packed.world_origin.astype(np.float64), float(packed.world_scale)
O, D = o[0].astype(np.float64), d[0].astype(np.float64)
for t in (X, Y):
    v = packed.vertices[packed.triangles[t]].astype(np.float64)
    e1, e2 = v[1] - v[0], v[2] - v[0]
    p = np.cross(D, e2); det = e1.dot(p); tv = O - v[0]; u = tv.dot(p) / det; q = np.cross(tv, e1); vv = D.dot(q) / det
    tt = e2.dot(q) / det
    w = nodes[np.flatnonzero(leaf)[np.flatnonzero(ids == t)[0]], :3]
    lo, hi = wo + (w & 0xFFFF) * ws, wo + (w >> 16) * ws
    with np.errstate(divide='ignore', invalid='ignore'):
        t0, t1 = (lo - O) / D, (hi - O) / D
    tmin, tmax = np.minimum(t0, t1).max(), np.maximum(t0, t1).min()
    out['tri_%d' % t] = dict(t=tt, u=u, v=vv, box_entry=float(tmin), box_exit=float(tmax), lo=lo.tolist(), hi=hi.tolist())
gdet = gpu.GPUDetector(geo)
NTPB, MAXB = 512, 1024
for n in (1 << 17, 4000):
    pp = Photons(np.repeat(o, n, 0), np.repeat(d, n, 0), np.tile(np.float32([[1, 0, 0]]), (n, 1)), np.full(n, 420.0, np.float32))
    res = []
    for rep in range(4):
        gp = gpu.GPUPhotons(pp, copy_flags=True, copy_triangles=False, copy_weights=False)
        rng = gpu.get_rng_states(NTPB * MAXB, seed=1)
        gp.propagate(gdet, rng, nthreads_per_block=NTPB, max_blocks=MAXB, max_steps=1)
        lh = gp.get().last_hit_triangles
        vals, cnt = np.unique(lh, return_counts=True)
        res.append({int(a): int(b) for a, b in zip(vals, cnt)})
    out['copies_%d' % n] = res
# the ray among its real neighbours: photons I-2^16 .. I+2^16 of the batch, one step
lo_i = I - (1 << 16)
sub = ph[lo_i:lo_i + (1 << 17)]
res = []
for rep in range(6):
    gp = gpu.GPUPhotons(sub, copy_flags=True, copy_triangles=False, copy_weights=False)
    rng = gpu.get_rng_states(NTPB * MAXB, seed=1)
    gp.propagate(gdet, rng, nthreads_per_block=NTPB, max_blocks=MAXB, max_steps=1)
    res.append(int(gp.get().last_hit_triangles[I - lo_i]))
out['among_neighbours'] = res
dd = ga.to_gpu(np.full(1, -7.0, np.float32))
go, gd = ga.to_gpu(o.reshape(-1)), ga.to_gpu(dn.reshape(-1))
_native.call('chr_distance_to_mesh', gdet._handle, 1, go.gpudata, gd.gpudata, dd.gpudata, current_stream())
torch.cuda.synchronize()
out['distance_to_mesh'] = float(dd.get()[0])
print(json.dumps(out))
