"""bench.py's multi-rank scaffolding on CPU (gloo, world size 2), the code the
driver's N>1 bench runs around the propagate step: rank 0 builds the geometry
and fills the node-local cache while the other ranks wait at a barrier and
then load it; per-rank RNG subsequences are disjoint; the timed loop brackets
its steps with barriers and reports the MAX over ranks; each step SUM-reduces
the per-channel hit counts (chroma.gpu.shard.allreduce_channel_counts).  The
propagate itself needs a GPU and is covered by the -m gpu tests."""
import os
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_usable_cpus():
    sys.path.insert(0, ROOT)
    import bench
    return bench.usable_cpus()


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, 'chroma-lite_amd'))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%d' % port, rank=rank, world_size=world)
    try:
        import bench
        from chroma.gpu import shard
        cache = os.path.join(out_dir, 'cache')
        det, setup = bench.shared_geometry('small', cache, rank, dist)
        from chroma.gpu import wide_bvh
        from chroma.gpu.packing import PackedGeometry
        src = wide_bvh.obtain(det.bvh, PackedGeometry(det))[1]
        md5 = int(det.mesh.md5()[:12], 16)
        nch = det.num_channels()
        counts = torch.zeros(nch, dtype=torch.int32)
        reduced = {}

        def run(m):   # m steps per call, as bench.py's pipelined groups
            out = []
            for _ in range(m):
                time.sleep(0.02 * (rank + 1))               # rank 1 is the slow one
                counts.fill_(0)
                counts[rank % nch] = 3 + rank                # this rank's "hits"
                reduced['c'] = shard.allreduce_channel_counts(counts)
                out.append(rank)
            return out

        elapsed, per_step, results = bench.timed_loop(run, 3, 1, dist, lambda: None, group=2)
        c = reduced['c'].numpy()
        res = np.array([elapsed, sum(per_step), md5, nch, bench.rng_first_subsequence(rank, 524288),
                        c[0], c[1 % nch], c.sum(), len(results),
                        # rank 0 built the traversal BVH before the barrier (it is then in memory);
                        # rank 1 loaded it from the cache rank 0 filled
                        {'built': 1, 'memory': 2, 'cache': 3}[src],
                        {'built': 1, 'cache': 3}.get(setup.get('wide_bvh_prepare_source'), 0)],
                       dtype=np.float64)
        np.save(os.path.join(out_dir, 'r%d.npy' % rank), res, allow_pickle=False)
    finally:
        dist.destroy_process_group()


def test_bench_world2_scaffolding(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(os.path.join(str(tmp_path), 'r%d.npy' % r)) for r in range(2))
    # one geometry, built once by rank 0 into the shared cache, loaded by rank 1
    assert r0[2] == r1[2] and r0[3] == r1[3]
    assert os.path.isdir(os.path.join(str(tmp_path), 'cache'))
    # the traversal BVH: built once by rank 0 before the barrier, loaded from the cache by rank 1
    assert r0[10] == 1 and r0[9] == 2 and r1[9] == 3
    # timed region: max over ranks -> identical on both, at least the slow rank's 3 steps
    assert r0[0] == r1[0] and r0[0] >= 3 * 0.04 - 1e-3
    assert r1[1] >= 3 * 0.04 - 1e-3
    # disjoint RNG subsequences: rank r starts at r * nslots
    assert (r0[4], r1[4]) == (0, 524288)
    # the per-step channel reduce: rank 0 put 3 in channel 0, rank 1 put 4 in channel 1
    for r in (r0, r1):
        assert r[5] == 3 and r[6] == 4 and r[7] == 7 and r[8] == 3


def _stub_bench(args, env_extra=None, timeout=120, full=True):
    """Run tests/bench_stub_main.py (bench.py with a CPU stand-in workload) as
    the driver would run bench.py --full (full=False: a plain run), with a fresh
    node-local cache; returns (returncode, parsed line or None, stderr)."""
    import json
    import subprocess
    import tempfile
    if '--cache-dir' not in args:
        args = list(args) + ['--cache-dir', tempfile.mkdtemp(prefix='bench_stub_cache_')]
    if full:
        args = list(args) + ['--full']
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR',
                                                            'MASTER_PORT')}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'bench_stub_main.py')] + args,
                       capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    return p.returncode, (json.loads(lines[-1]) if lines else None), p.stderr


def test_bench_gpus2_spawns_two_ranks():
    """`bench.py --gpus 2` without WORLD_SIZE starts two rank processes (the
    VERDICT r02 item 1 gap: --gpus was parsed and ignored), and the N=2 line
    carries n_gpus 2, the ranks seen, every rank's parity and roofline."""
    rc, line, err = _stub_bench(['--gpus', '2', '--steps', '4', '--warmup', '1', '--photons', '1000',
                                 '--pipeline-depth', '2', '--sequential-steps', '2', '--detector', 'small'])
    assert rc == 0, err
    assert line['n_gpus'] == 2 and line['scaling'] == 'weak'
    d = line['detail']
    assert d['ranks_seen'] == 2 and [r['rank'] for r in d['ranks']] == [0, 1]
    assert line['value'] == pytest.approx(2 * 1000 * 4 / (line['ms_per_step'] * 4 / 1e3))
    # rank 1 (sleeps 20 ms per step) sets the max-over-ranks time
    assert line['ms_per_step'] >= 20.0
    assert d['channel_hits_all_ranks'] == 1 + 2        # rank 0 put 1, rank 1 put 2 (SUM over ranks)
    assert d['sequential']['steps'] == 2 and d['sequential']['photons_per_s'] > 0
    par = line['parity']
    assert par['all_ranks_equal'] and [p['rank'] for p in par['per_rank']] == [0, 1]
    assert par['per_rank'][0]['full'] and not par['per_rank'][1]['full']
    assert par['per_rank'][1]['rng_first_subsequence'] == 524288
    # rank 1's sample went to rank 0, which ran its oracle check
    assert par['per_rank'][1]['oracle_on_rank'] == 0 and par['per_rank'][1]['n'] == 1000
    for r in d['ranks']:
        assert r['host_rss_gb'] > 0 and r['host_peak_rss_gb'] >= r['host_rss_gb'] - 1e-3
        assert set(r['setup']) >= {'geometry_s', 'upload_s', 'setup_s', 'host_rss_gb'}
    rl = line['roofline']
    assert [r['rank'] for r in rl['per_rank']] == [0, 1]
    # rank 1's launches: 2 ms+1 over 2 launches of 1000 rays / step -> its own frac
    assert rl['per_rank'][1]['avg_launch_ms'] == pytest.approx(1.5)
    assert line['cpu_baseline']['cores'] >= 1


def test_bench_gpus8_line():
    """The driver's 8-GPU command (`bench.py --gpus 8`), rehearsed with 8 gloo ranks:
    8 ranks seen, the max-over-ranks time, every rank's parity (ranks 1-7 checked by
    rank 0's oracle on their own RNG subsequences), roofline and host memory /
    setup fields -- what a first 8-GPU run needs to be diagnosable."""
    rc, line, err = _stub_bench(['--gpus', '8', '--steps', '2', '--warmup', '1', '--photons', '1000',
                                 '--pipeline-depth', '2', '--sequential-steps', '1', '--detector', 'small',
                                 '--rank-parity-photons', '500'], timeout=300)
    assert rc == 0, err
    assert line['n_gpus'] == 8
    d = line['detail']
    assert d['ranks_seen'] == 8 and [r['rank'] for r in d['ranks']] == list(range(8))
    assert line['ms_per_step'] >= 80.0                  # rank 7 sleeps 80 ms per step: the max over ranks
    assert line['value'] == pytest.approx(8 * 1000 * 2 / (line['ms_per_step'] * 2 / 1e3))
    assert d['channel_hits_all_ranks'] == sum(1 + r for r in range(8))
    par = line['parity']
    assert par['all_ranks_equal'] and [p['rank'] for p in par['per_rank']] == list(range(8))
    for r, p in enumerate(par['per_rank']):
        assert p['rng_first_subsequence'] == r * 524288 and p['oracle_on_rank'] == 0
        assert p['n'] == (100 if r == 0 else 500)
    assert [r['rank'] for r in line['roofline']['per_rank']] == list(range(8))
    for r in d['ranks']:
        assert r['host_rss_gb'] > 0 and 'setup_s' in r['setup']
    # a fresh cache: rank 0 builds the traversal BVH once before the barrier, ranks 1-7
    # load it from the node-local cache (no 8 concurrent builds), each with its share
    # of the job's cores
    s0 = d['ranks'][0]['setup']
    assert s0['wide_bvh_prepare_source'] == 'built' and s0['wide_bvh_source'] == 'memory'
    for r in d['ranks'][1:]:
        assert r['setup']['wide_bvh_source'] == 'cache' and 'wide_bvh_prepare_source' not in r['setup']
    assert all(r['setup']['host_threads'] == max(1, bench_usable_cpus() // 8) for r in d['ranks'])


def test_bench_total_photons_is_strong_scaling():
    rc, line, err = _stub_bench(['--gpus', '2', '--steps', '2', '--warmup', '0', '--total-photons', '1001',
                                 '--sequential-steps', '0', '--detector', 'small'])
    assert rc == 0, err
    assert line['scaling'] == 'strong' and line['config']['total_photons'] == 1001
    assert [r['photons_per_step'] for r in line['detail']['ranks']] == [500, 501]
    assert line['value'] == pytest.approx(1001 * 2 / (line['ms_per_step'] * 2 / 1e3))
    assert line['detail']['sequential'] is None


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times its --steps steps and nothing else: no
    sequential, slot-timing or counting pass, no CPU baseline, parity, roofline
    or geometry hashes; the headline fields are there.  --dump-outputs DIR
    writes the last timed step's outputs as float32 / float64 .npy, the same
    from run to run."""
    dirs = [str(tmp_path / 'a'), str(tmp_path / 'b')]
    for d in dirs:
        rc, line, err = _stub_bench(['--gpus', '1', '--steps', '3', '--warmup', '1', '--photons', '1000',
                                     '--detector', 'small', '--dump-outputs', d], full=False)
        assert rc == 0, err
        assert line['full'] is False and line['steps'] == 3 and len(line['detail']['step_ms']) == 3
        assert line['unit'] == 'photons/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
        assert line['value'] == pytest.approx(1000 * 3 / (line['ms_per_step'] * 3 / 1e3))
        assert line['ms_per_step'] >= 10.0                  # the stand-in step sleeps 10 ms
        assert line['parity'] is None and line['cpu_baseline'] is None and line['roofline'] is None
        assert line['geometry_md5_match'] is None
        assert line['detail']['sequential'] is None and line['detail']['slot_timing_pass'] is None
        # the stand-in saw the warm-up (2 steps for a pipelined run) and the timed steps only
        assert line['detail']['stub_calls'] == [[2, True], [3, True]]
    names = sorted(os.listdir(dirs[0]))
    assert names == ['channel_hit_counts.npy', 'flags.npy', 'photon_index.npy', 'pos.npy']
    assert sorted(os.listdir(dirs[1])) == names
    for n in names:
        a, b = np.load(os.path.join(dirs[0], n)), np.load(os.path.join(dirs[1], n))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    assert np.load(os.path.join(dirs[0], 'pos.npy')).dtype == np.float32
    assert np.array_equal(np.load(os.path.join(dirs[0], 'flags.npy')), np.full(1000, 4.0))
    assert np.array_equal(np.load(os.path.join(dirs[0], 'channel_hit_counts.npy')), [1.0, 0.0, 0.0, 0.0])


def test_bench_dump_sample_is_fixed():
    """--dump-outputs keeps every photon of a small batch and a fixed, seeded,
    ascending sample of a large one (at most 64 MB of float32 / float64 in all)."""
    sys.path.insert(0, ROOT)
    import bench
    assert np.array_equal(bench.dump_sample(1000), np.arange(1000))
    a, b = bench.dump_sample(10_000_000), bench.dump_sample(10_000_000)
    assert np.array_equal(a, b) and len(a) == bench.DUMP_PHOTONS and len(np.unique(a)) == len(a)
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 10_000_000
    # 12 float32 + 3 float64 fields per photon, the indices, the 29k detector's channel counts
    assert bench.DUMP_PHOTONS * (12 * 4 + 3 * 8 + 8) + 29007 * 8 <= 64e6


def test_bench_prime_cache_leaves_room_on_disk(tmp_path, monkeypatch):
    """bench.prime_cache (what build() runs on a GPU machine) fills the cache the
    benchmark and the GPU tests share -- one copy -- and refuses to write an entry
    that would leave the disk with less than half the entry's size again."""
    import collections
    import shutil
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.delenv('CHROMA_BENCH_CACHE', raising=False)
    assert bench.default_cache_dir() == '/tmp/chroma_bench_cache'
    monkeypatch.setenv('CHROMA_BENCH_CACHE', str(tmp_path / 'env'))
    assert bench.default_cache_dir() == str(tmp_path / 'env')
    monkeypatch.setenv('CHROMA_BENCH_MEMAVAILABLE_GB', '500')
    usage = collections.namedtuple('usage', 'total used free')
    monkeypatch.setattr(shutil, 'disk_usage', lambda p: usage(100e9, 80e9, 20e9))
    cache = str(tmp_path / 'cache')
    r = bench.prime_cache('29k', cache)       # 16 GB entry, 20 GB free: not written
    assert r['primed'] is False and '20.0 GB free' in r['reason'] and not os.path.exists(cache)
    r = bench.prime_cache('small', cache)
    assert r['primed'] and r['wide_bvh_source'] == 'built' and r['cache_dir'] == cache
    monkeypatch.setattr(shutil, 'disk_usage', lambda p: usage(100e9, 100e9, 0.0))
    r = bench.prime_cache('small', cache)     # the entry is there: nothing to write
    assert r['primed'] and r['wide_bvh_source'] == 'cache'


def test_bench_failed_rank_fails_the_run():
    rc, line, err = _stub_bench(['--gpus', '2', '--steps', '2', '--detector', 'small'], {'STUB_FAIL_RANK': '1'})
    assert rc != 0 and line is None
    assert 'rank 1 exited' in err


def test_bench_world_size_mismatch_is_refused():
    rc, line, err = _stub_bench(['--gpus', '4', '--steps', '1', '--detector', 'small'], {'WORLD_SIZE': '1'})
    assert rc != 0 and line is None and 'WORLD_SIZE=1' in err


def test_bench_parity_failure_exits_nonzero():
    """A parity check that fails (here rank 1's sample, checked by rank 0's
    oracle) still prints the line -- parity.ok false, the failing rank named --
    and the run exits non-zero (the bench enforces the
    contract instead of only reporting it)."""
    rc, line, err = _stub_bench(['--gpus', '2', '--steps', '2', '--warmup', '1', '--photons', '1000',
                                 '--sequential-steps', '0', '--detector', 'small'], {'STUB_PARITY_FAIL_RANK': '1'})
    assert rc != 0 and 'PARITY FAILED' in err
    assert line is not None and line['parity']['ok'] is False
    assert [p['ok'] for p in line['parity']['per_rank']] == [True, False]
    rc, line, err = _stub_bench(['--gpus', '2', '--steps', '2', '--warmup', '1', '--photons', '1000',
                                 '--sequential-steps', '0', '--detector', 'small', '--allow-parity-failure'],
                                {'STUB_PARITY_FAIL_RANK': '1'})
    assert rc == 0 and line['parity']['ok'] is False


def test_bench_host_memory_preflight():
    """The first 8-GPU run fails loudly rather than by an out-of-memory kill
    (VERDICT r05 item 7): 8 ranks of the 29k detector need ~64 GB on rank 0
    (cold build + oracle) and ~26 GB on each other rank; with 150 GB available
    the run is refused before any rank builds geometry, with the numbers in the
    message.  A job that fits carries the pre-flight record in the line."""
    sys.path.insert(0, ROOT)
    import bench
    pf = bench.preflight_host_memory('29k', 8, avail=150e9)
    assert not pf['fits'] and pf['need_gb'] == 64.0 + 7 * 26.0
    assert bench.preflight_host_memory('29k', 8, avail=300e9)['fits']
    assert bench.preflight_host_memory('29k', 1, avail=70e9)['fits']
    rc, line, err = _stub_bench(['--gpus', '8', '--steps', '1', '--detector', '29k'],
                                {'CHROMA_BENCH_MEMAVAILABLE_GB': '150'}, timeout=300)
    assert rc != 0 and line is None
    assert 'pre-flight refused' in err and '246 GB' in err and '150 GB' in err
    rc, line, err = _stub_bench(['--gpus', '2', '--steps', '1', '--warmup', '0', '--photons', '1000',
                                 '--sequential-steps', '0', '--detector', 'small'],
                                {'CHROMA_BENCH_MEMAVAILABLE_GB': '150'})
    assert rc == 0, err
    pf = line['detail']['preflight']
    assert pf['fits'] and pf['local_ranks'] == 2 and pf['need_gb'] == 3.0 and pf['available_gb'] == 150.0


def test_bench_float_parity_rule():
    """bench.py's float contract (PARITY_RULE): pos within 1e-5 * max(|oracle|, 1 mm),
    t / wavelengths within 1e-5 * |oracle|; the worst photon is named with its batch,
    values, flags and last hit."""
    sys.path.insert(0, ROOT)
    import bench
    n = 10
    gf = hf = np.full(n, 4, np.uint32)
    gl = hl = np.arange(n, dtype=np.int32)
    want = np.zeros((n, 3), np.float32)
    want[:, 0] = 0.3
    got = want.copy()
    got[2, 0] += 1e-6                  # 3e-6 relative, but far below 1e-5 * 1 mm
    r = bench.float_contract(got, want, 'pos', [5, 5], gf, hf, gl, hl)
    assert r['violations'] == 0 and r['differing'] == 1 and r['worst']['index'] == 2
    got[7, 1] = 2e-5                   # 2e-5 mm off a coordinate 0: beyond 1e-5 mm
    r = bench.float_contract(got, want, 'pos', [5, 5], gf, hf, gl, hl)
    assert r['violations'] == 1 and r['worst']['index'] == 7 and r['worst']['batch'] == 1
    assert r['worst']['index_in_batch'] == 2 and r['worst']['over_tolerance'] > 1.0
    t = np.linspace(1.0, 2.0, n)
    t2 = t.copy()
    t2[4] *= 1 + 2e-5
    r = bench.float_contract(t2, t, 't', [5, 5], gf, hf, gl, hl)
    assert r['violations'] == 1 and r['worst']['index'] == 4 and r['worst']['last_hit_oracle'] == 4
    r = bench.float_contract(t, t, 't', [5, 5], gf, hf, gl, hl)
    assert r == {'violations': 0, 'differing': 0, 'max_abs': 0.0}


def test_bench_photons_at_max_steps():
    """detail.tail_launch[i].photons_at_max_steps: photons of each
    batch whose history holds no terminal bit (NO_HIT, BULK_ABSORB, SURFACE_DETECT,
    SURFACE_ABSORB, NAN_ABORT) -- the ones propagate.cu's loop left alive at max_steps;
    scattering / reflection bits and the upper 16 bits do not count as terminal."""
    sys.path.insert(0, ROOT)
    import types
    import bench
    wl = object.__new__(bench.PropagateWorkload)

    def batch(flags):
        t = torch.tensor(np.asarray(flags, np.uint32).view(np.int32))
        return types.SimpleNamespace(flags=types.SimpleNamespace(tensor=t))
    wl.pool = [batch([0x10, 0x2, 0x4 | 0x10, 0x20, 0x10000]), batch([0x1, 0x8, 0x8000, 0x4]), batch([])]
    assert wl.at_max_steps(2) == [3, 0]
    assert wl.at_max_steps(3) == [3, 0, 0]
    assert wl.at_max_steps(4) == [None] * 4       # more batches than the pool holds
    assert wl.at_max_steps(0) == []
