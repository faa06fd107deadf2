"""Pin the oracle's tracked mode (oracle.propagate(track=True),
oracle.propagate_tracked) on the CPU against the already-pinned untracked loop.

track=True is the reference's policy (chroma/gpu/photon.py:261-264): every
host step is one step whatever the live count.  The untracked policy takes
single steps too while nthreads_per_block*128 or more photons are queued, so
at a launch shape whose threshold every compared step stays above, the two
must give identical photons and RNG slot states."""
import numpy as np
import pytest

import oracle
import scenes

DEAD = 0x800F      # NO_HIT | BULK_ABSORB | SURFACE_DETECT | SURFACE_ABSORB | NAN_ABORT (device bit 15)


@pytest.fixture(scope='module')
def scene():
    from chroma import loader
    from chroma.gpu.packing import PackedGeometry
    geo = loader.create_geometry_from_obj(scenes.physics_scene())
    return geo, PackedGeometry(geo)


def _equal(a, b):
    for f in oracle.HostPhotons.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not np.array_equal(x, y):
            return False
    return True


def test_tracked_equals_untracked_above_threshold(scene):
    """(ntpb, max_blocks) = (1, 4096): the untracked loop finishes in one
    launch only below 1*128 queued photons.  12000 photons on the physics
    scene keep every step up to the 6th above that (asserted), so tracked and
    untracked runs of 1..6 steps are the same computation."""
    geo, packed = scene
    photons = scenes.photon_sources(12000, seed=61)
    ntpb, max_blocks, nslots = 1, 4096, 4096
    initial = np.arange(12000, dtype=np.uint32)
    prev_alive = np.ones(12000, bool)
    for max_steps in range(1, 7):
        plain = oracle.HostPhotons(photons)
        st_plain = oracle.rng_init(nslots, seed=4)
        s_plain = oracle.propagate(packed, plain, st_plain, nslots, ntpb, max_blocks, max_steps)
        tracked = oracle.HostPhotons(photons)
        st_tracked = oracle.rng_init(nslots, seed=4)
        s_tracked = oracle.propagate(packed, tracked, st_tracked, nslots, ntpb, max_blocks, max_steps, track=True)
        # non-vacuity: the queue entering this run's last step (the live photons of
        # the untracked run one step shorter) is at or above the 128-photon threshold
        assert prev_alive.sum() >= ntpb * 128, (max_steps, int(prev_alive.sum()))
        assert s_plain['host_steps'] == max_steps and s_tracked['host_steps'] == max_steps
        assert _equal(plain, tracked), 'photons differ at max_steps=%d' % max_steps
        assert np.array_equal(st_plain, st_tracked), 'RNG states differ at max_steps=%d' % max_steps
        ids = s_tracked['step_ids']
        assert len(ids) == max_steps + 1
        assert np.array_equal(ids[0], initial) and np.array_equal(ids[1], initial)
        # the queue that entered the last step: the previous run's survivors, in input order
        assert np.array_equal(ids[max_steps], initial[prev_alive])
        prev_alive = (plain.flags & DEAD) == 0


def test_tracked_takes_single_steps_below_threshold(scene):
    """Below the threshold the policies differ: the untracked loop ends in one
    multi-step launch, the tracked one goes on stepping; the RNG slot a photon
    draws from changes with every compaction, so the photons differ."""
    geo, packed = scene
    photons = scenes.photon_sources(1500, seed=61)
    plain = oracle.HostPhotons(photons)
    s_plain = oracle.propagate(packed, plain, oracle.rng_init(4096, seed=4), 4096, 64, 64, 8)
    tracked = oracle.HostPhotons(photons)
    s_tracked = oracle.propagate(packed, tracked, oracle.rng_init(4096, seed=4), 4096, 64, 64, 8, track=True)
    assert s_plain['host_steps'] == 1 and s_tracked['host_steps'] == 8
    assert not _equal(plain, tracked)


def test_propagate_tracked_entries(scene):
    """The entry convention of the reference (photon.py:255-257, 270-272): entry
    0 the whole first queue (clones interleaved) with the input photons; entry
    k the queue that entered step k with its photons' state after k steps; the
    list ends at max_steps or once a step leaves nobody queued."""
    geo, packed = scene
    photons = scenes.photon_sources(700, seed=62)
    n, ncopies, max_steps = 700, 2, 5
    ids, steps, final, rng = oracle.propagate_tracked(packed, photons, 9, 4096, 64, 64, max_steps, ncopies=ncopies)
    assert len(ids) == len(steps) == max_steps + 1
    q0 = np.empty(n * ncopies, np.uint32)
    q0[0::2] = np.arange(n)
    q0[1::2] = np.arange(n) + n
    assert np.array_equal(ids[0], q0) and np.array_equal(ids[1], q0)
    assert (ids[0] >= n).sum() == n
    first = oracle._replicated(photons, ncopies)
    for f in first.FIELDS:
        assert np.array_equal(getattr(steps[0], f), getattr(first, f)[q0]), f
    assert (steps[0].flags == 0).all()
    for k in range(1, max_steps + 1):
        # a fresh k-step tracked run gives the state entry k holds
        host = oracle._replicated(photons, ncopies)
        oracle.propagate(packed, host, oracle.rng_init(4096, seed=9), 4096, 64, 64, k, ncopies=ncopies, track=True)
        for f in host.FIELDS:
            want = np.ascontiguousarray(getattr(host, f)[ids[k]])
            got = getattr(steps[k], f)
            assert got.dtype == want.dtype and got.shape == want.shape, f
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, f)
        if k < max_steps:    # the next queue: this step's survivors, order kept
            assert np.array_equal(ids[k + 1], ids[k][(steps[k].flags & DEAD) == 0])
    assert _equal(final, host)
    # every photon's last entry is its final state
    last = {}
    for k, q in enumerate(ids):
        for j, pid in enumerate(q):
            last[int(pid)] = (k, j)
    fl = np.array([steps[k].flags[j] for pid, (k, j) in sorted(last.items())])
    assert np.array_equal(fl, final.flags)


def test_propagate_tracked_stops_when_nobody_is_left(scene):
    """Photons that all leave the queue at step 1 (origins outside the world
    looking away: NO_HIT).  The reference breaks out of its loop
    (photon.py:285-286): two entries.  max_steps = 0: one entry, nothing run."""
    from chroma.event import Photons
    geo, packed = scene
    n = 300
    pos = np.tile(np.array([0.0, 0.0, 5000.0], np.float32), (n, 1))
    dir = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (n, 1))
    pol = np.tile(np.array([1.0, 0.0, 0.0], np.float32), (n, 1))
    photons = Photons(pos, dir, pol, np.full(n, 400.0, np.float32))
    ids, steps, final, rng = oracle.propagate_tracked(packed, photons, 9, 4096, 64, 64, 10)
    assert len(ids) == 2 and len(ids[1]) == n
    assert (steps[1].flags == 1).all() and (final.flags == 1).all()
    assert np.array_equal(rng, oracle.rng_init(4096, seed=9))      # a miss draws nothing
    ids0, steps0, final0, rng0 = oracle.propagate_tracked(packed, photons, 9, 4096, 64, 64, 0)
    assert len(ids0) == 1 and (final0.flags == 0).all() and np.array_equal(rng0, oracle.rng_init(4096, seed=9))
