"""The host side of a photon library: the voxel grid whose cells are the
library's sources, and the entries -- per event, which sources were lit, by how
many photons and when -- that chroma.gpu.library looks up.  Nothing here needs
a device.

    grid = VoxelGrid((-500, -500, -500), (500, 500, 500), (10, 10, 10))
    lib = sim.build_library(grid, water, photons_per_voxel=100000, tbins=50, trange=(0, 100))
    entries = entries_from_gensteps(grid, [steps_of_event_0, steps_of_event_1])
    mu = lib.expect(entries).get().mu          # (2, nchannels) expected charges
"""
import numpy as np

NO_SOURCE = 0xFFFFFFFF          # the source of a step outside the grid: counted in `skipped`
MAX_WORDS = 2 ** 31


class VoxelGrid(object):
    """An axis-aligned box [lo, hi) cut into shape = (nx, ny, nz) equal voxels.
    The voxel (ix, iy, iz) is source ix + nx*(iy + ny*iz)."""

    def __init__(self, lo, hi, shape):
        self.lo = np.asarray(lo, np.float64).reshape(3)
        self.hi = np.asarray(hi, np.float64).reshape(3)
        self.shape = tuple(int(n) for n in shape)
        if len(self.shape) != 3 or min(self.shape) <= 0:
            raise ValueError('shape must be three positive voxel counts')
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all() and (self.hi > self.lo).all()):
            raise ValueError('hi must be above lo on every axis')
        if self.nvoxels > MAX_WORDS:
            raise ValueError('%d voxels exceed 2^31 sources' % self.nvoxels)

    @property
    def nvoxels(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    def index(self, points):
        """The source ids (int64) of points (n, 3), -1 outside the box; in
        float64.  A point on a low face belongs to the voxel, one on a high
        face of the box is outside."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        n = np.asarray(self.shape, np.float64)
        with np.errstate(invalid='ignore'):
            x = (p - self.lo) / (self.hi - self.lo) * n
            inside = ((p >= self.lo) & (p < self.hi) & (x < n)).all(axis=1)
        i = np.where(inside[:, None], np.floor(np.where(inside[:, None], x, 0.0)), 0.0).astype(np.int64)
        ids = i[:, 0] + self.shape[0] * (i[:, 1] + self.shape[1] * i[:, 2])
        return np.where(inside, ids, -1)

    def centers(self):
        """The voxel centres (nvoxels, 3) float64, in source-id order."""
        ids = np.arange(self.nvoxels)
        nx, ny, _ = self.shape
        i = np.stack([ids % nx, (ids // nx) % ny, ids // (nx * ny)], axis=1)
        return self.lo + (i + 0.5) * (self.hi - self.lo) / np.asarray(self.shape, np.float64)

    def flashes(self, material, nphotons, wavelength_range=(380.0, 500.0)):
        """A Gensteps of one isotropic flash of nphotons photons at every voxel
        centre, its evidx the voxel's source id."""
        from chroma import gensteps as gs
        rec = np.zeros(self.nvoxels, gs.GENSTEP_DTYPE)
        index = isinstance(material, (int, np.integer))
        rec['kind'], rec['nphotons'] = gs.ISOTROPIC, int(nphotons)
        rec['material'] = int(material) if index else 0
        rec['evidx'] = np.arange(self.nvoxels, dtype=np.uint32)
        rec['x0'] = self.centers().astype(np.float32)
        rec['wl_lo'], rec['wl_hi'] = wavelength_range
        return gs.Gensteps(rec, [None if index else material] * self.nvoxels)

    def __eq__(self, other):
        return isinstance(other, VoxelGrid) and self.shape == other.shape and \
            np.array_equal(self.lo, other.lo) and np.array_equal(self.hi, other.hi)


class LibraryEntries(object):
    """The CSR table of chr_library_entries: event e owns entries offsets[e] ..
    offsets[e+1]-1; per entry the source (uint32), the photons made there
    (uint32) and when (float32)."""

    def __init__(self, offsets, source, nphotons, t):
        def exact(a, dtype, name):
            a = np.asarray(a)
            out = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            if dtype != np.float32 and a.size and not np.array_equal(out.astype(np.float64), a.reshape(-1)):
                raise ValueError('%s does not fit uint32' % name)
            return out
        self.offsets = exact(offsets, np.uint32, 'offsets')
        self.source = exact(source, np.uint32, 'source')
        self.nphotons = exact(nphotons, np.uint32, 'nphotons')
        self.t = exact(t, np.float32, 't')
        if len(self.offsets) < 1:
            raise ValueError('offsets needs nevents + 1 words')
        if not (len(self.source) == len(self.nphotons) == len(self.t)):
            raise ValueError('source, nphotons and t differ in length')
        if (np.diff(self.offsets.astype(np.int64)) < 0).any():
            raise ValueError('offsets not ascending')
        if int(self.offsets[-1]) > len(self.source):
            raise ValueError('offsets reach entry %d of %d' % (int(self.offsets[-1]), len(self.source)))

    @property
    def nevents(self):
        return len(self.offsets) - 1

    @property
    def nentries(self):
        return int(self.offsets[-1]) - int(self.offsets[0])


def entries_from_gensteps(grid, gensteps_list):
    """One event per Gensteps, one entry per step, in order: the source is the
    voxel of the step's midpoint x0 + dx/2 (NO_SOURCE outside the grid, so the
    lookup counts it in `skipped`), the time t0 + dt/2 in float32."""
    parts = [g.steps for g in gensteps_list]
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    if parts and offsets[-1] > 0:
        rec = np.concatenate(parts)
        mid = rec['x0'].astype(np.float64) + 0.5 * rec['dx'].astype(np.float64)
        ids = grid.index(mid)
        source = np.where(ids < 0, NO_SOURCE, ids).astype(np.uint32)
        t = rec['t0'] + np.float32(0.5) * rec['dt']
        return LibraryEntries(offsets, source, rec['nphotons'], t.astype(np.float32))
    return LibraryEntries(offsets, [], [], [])
