"""Gensteps: compact records of where light is made, turned into photons on
the device (chroma.gpu.generate_photons) or, bit for bit the same, on the host
(generate_photons_host, no GPU needed).

A genstep says "nphotons photons start along the segment x0 .. x0 + dx, at
times t0 .. t0 + dt, in this material" -- what a charged-particle simulation
knows after one step.  The yield (Birks, dE/dx, the Frank-Tamm integral) is the
caller's: it gives nphotons.  The record is the C ABI's chr_genstep
(include/chroma_amd.h, 64 bytes); INTEGRATION.md documents the draw order.

    from chroma import gensteps
    gs = gensteps.cherenkov_step(water, 500, x0=(0, 0, 0), dx=(0, 0, 30), beta=0.99, t0=0.0, dt=0.1)
    gs += gensteps.scintillation_step(scint, 2000, x0=(0, 0, 0), dx=(0, 0, 30), component=0)
    for ev in sim.simulate([gs]): ...
"""
import ctypes

import numpy as np

from chroma import event

ISOTROPIC, SCINTILLATION, CHERENKOV = 0, 1, 2

GENSTEP_DTYPE = np.dtype([('kind', '<u4'), ('nphotons', '<u4'), ('material', '<u4'), ('evidx', '<u4'),
                          ('x0', '<f4', (3,)), ('t0', '<f4'), ('dx', '<f4', (3,)), ('dt', '<f4'),
                          ('wl_lo', '<f4'), ('wl_hi', '<f4'), ('beta', '<f4'), ('component', '<u4')])
assert GENSTEP_DTYPE.itemsize == 64


class Gensteps(object):
    """A sequence of gensteps: `steps` (GENSTEP_DTYPE records) and, per step,
    the Material object the step names or None when `steps['material']`
    already holds the index into the geometry's materials
    (Geometry.unique_materials order, wire-plane materials after them).
    `a + b` concatenates; len() is the number of photons they make."""

    def __init__(self, steps=None, materials=None):
        self.steps = np.zeros(0, GENSTEP_DTYPE) if steps is None else \
            np.ascontiguousarray(np.atleast_1d(steps), dtype=GENSTEP_DTYPE)
        # the named Material objects, each once, and per step its place in that list (-1: an index)
        self._objects = []
        self._codes = np.full(len(self.steps), -1, np.int32)
        if materials is not None:
            materials = list(materials)
            if len(materials) != len(self.steps):
                raise ValueError('one material entry per step')
            seen = {}
            for i, m in enumerate(materials):
                if m is None:
                    continue
                if id(m) not in seen:
                    seen[id(m)] = len(self._objects)
                    self._objects.append(m)
                self._codes[i] = seen[id(m)]

    @property
    def materials(self):
        return [None if c < 0 else self._objects[c] for c in self._codes]

    @property
    def nsteps(self):
        return len(self.steps)

    @property
    def nphotons(self):
        return int(self.steps['nphotons'].astype(np.uint64).sum())

    def __len__(self):
        return self.nphotons

    def __add__(self, other):
        if not isinstance(other, Gensteps):
            return NotImplemented
        return Gensteps.join([self, other])

    @staticmethod
    def join(parts):
        parts = list(parts)
        out = Gensteps(np.concatenate([p.steps for p in parts]) if parts else None)
        codes, seen = [], {}
        for p in parts:
            remap = np.full(len(p._objects) + 1, -1, np.int32)      # the last entry serves code -1
            for j, m in enumerate(p._objects):
                if id(m) not in seen:
                    seen[id(m)] = len(out._objects)
                    out._objects.append(m)
                remap[j] = seen[id(m)]
            codes.append(remap[p._codes])
        if codes:
            out._codes = np.concatenate(codes).astype(np.int32)
        return out

    def records(self, material_objects=None):
        """The records with every material resolved to its index in
        `material_objects` (matched by identity), ready for the C ABI."""
        rec = self.steps.copy()
        if not self._objects or not (self._codes >= 0).any():
            return rec
        if material_objects is None:
            raise ValueError('the steps name Material objects: a geometry is needed to resolve them')
        index = np.zeros(len(self._objects), np.uint32)
        for j, m in enumerate(self._objects):
            if not (self._codes == j).any():
                continue
            for k, x in enumerate(material_objects):
                if x is m:
                    index[j] = k
                    break
            else:
                raise ValueError('material %r is not in the geometry' % (getattr(m, 'name', m),))
        named = self._codes >= 0
        rec['material'][named] = index[self._codes[named]]
        return rec


def _step(kind, material, nphotons, x0, dx, t0, dt, wl_lo=0.0, wl_hi=0.0, beta=0.0, component=0, evidx=0):
    rec = np.zeros(1, GENSTEP_DTYPE)
    index = isinstance(material, (int, np.integer))
    rec['kind'], rec['nphotons'], rec['evidx'] = kind, int(nphotons), int(evidx)
    rec['material'] = int(material) if index else 0
    rec['x0'], rec['t0'], rec['dx'], rec['dt'] = np.asarray(x0, np.float32), t0, np.asarray(dx, np.float32), dt
    rec['wl_lo'], rec['wl_hi'], rec['beta'], rec['component'] = wl_lo, wl_hi, beta, int(component)
    return Gensteps(rec, [None if index else material])


def isotropic_flash(material, nphotons, x0=(0.0, 0.0, 0.0), dx=(0.0, 0.0, 0.0), t0=0.0, dt=0.0,
                    wavelength_range=(380.0, 500.0), evidx=0):
    """nphotons isotropic photons of uniform wavelength (chroma.photon_source.isotropic's
    distribution, drawn on the device), from a point or spread along a segment."""
    return _step(ISOTROPIC, material, nphotons, x0, dx, t0, dt, wavelength_range[0], wavelength_range[1],
                 evidx=evidx)


def scintillation_step(material, nphotons, x0, dx=(0.0, 0.0, 0.0), t0=0.0, dt=0.0, component=0, evidx=0):
    """nphotons scintillation photons: wavelength and emission delay from the
    material's comp_reemission_wvl_cdf / comp_reemission_time_cdf[component],
    isotropic direction."""
    return _step(SCINTILLATION, material, nphotons, x0, dx, t0, dt, component=component, evidx=evidx)


def cherenkov_step(material, nphotons, x0, dx, beta, t0=0.0, dt=0.0, wavelength_range=(200.0, 700.0), evidx=0):
    """nphotons Cherenkov photons of a particle of speed beta*c moving along dx:
    wavelengths from the Frank-Tamm spectrum (1 - 1/(beta n)^2) / wl^2 over
    wavelength_range, directions on the cone cos(theta) = 1/(beta n(wl))."""
    return _step(CHERENKOV, material, nphotons, x0, dx, t0, dt, wavelength_range[0], wavelength_range[1], beta,
                 evidx=evidx)


# ---------------------------------------------------------------- host twin
def rng_init_host(nslots, seed=1, offset=0, first_subsequence=0):
    """chroma.gpu.get_rng_states on the host: 6*nslots uint32, the device's SoA layout."""
    from chroma.gpu import _native
    st = np.zeros(6 * int(nslots), np.uint32)
    _native.call('chr_init_rng_host', st.ctypes.data, int(nslots), int(seed) & (2 ** 64 - 1),
                 int(first_subsequence), int(offset))
    return st


def _as_records(gensteps, material_objects):
    if isinstance(gensteps, Gensteps):
        return gensteps.records(material_objects)
    return np.ascontiguousarray(np.atleast_1d(gensteps), dtype=GENSTEP_DTYPE)


def count(gensteps):
    """Photons the records make (chr_gensteps_count)."""
    from chroma.gpu import _native
    rec = gensteps.steps if isinstance(gensteps, Gensteps) else _as_records(gensteps, None)
    total = ctypes.c_uint64()
    _native.call('chr_gensteps_count', rec.ctypes.data, len(rec), ctypes.byref(total))
    return total.value


def generate_photons_host(gensteps, packed, rng_states, first_photon=0, capacity=None):
    """The photons chroma.gpu.generate_photons makes, computed on the host
    (chr_generate_photons_host: the kernel's source built by the host compiler,
    bit-identical).  packed: a chroma.gpu.packing.PackedGeometry; rng_states:
    6*nslots uint32 (rng_init_host), advanced in place.  Returns
    (event.Photons of `capacity` photons -- those outside [first_photon,
    first_photon + n) left zero --, exhausted)."""
    from chroma.gpu import _native
    rec = _as_records(gensteps, getattr(packed, 'material_objects', None))
    n = int(rec['nphotons'].astype(np.uint64).sum())
    cap = min(first_photon + n if capacity is None else int(capacity), 2 ** 32 - 1)
    # a call the library will refuse (too many photons for the capacity or for one call) writes
    # nothing: it gets one-element arrays instead of the capacity's
    size = cap if n < 2 ** 31 and first_photon + n <= cap else 1
    arrays = dict(pos=np.zeros((size, 3), np.float32), dir=np.zeros((size, 3), np.float32),
                  pol=np.zeros((size, 3), np.float32), wavelengths=np.zeros(size, np.float32),
                  t=np.zeros(size, np.float32), weights=np.zeros(size, np.float32), flags=np.zeros(size, np.uint32),
                  last_hit_triangles=np.zeros(size, np.int32), evidx=np.zeros(size, np.uint32))
    desc = _native.PhotonsDesc(*[arrays[f].ctypes.data for f in ('pos', 'dir', 'pol', 'wavelengths', 't', 'weights',
                                                                  'flags', 'last_hit_triangles', 'evidx')])
    if not (isinstance(rng_states, np.ndarray) and rng_states.dtype == np.uint32 and rng_states.flags.c_contiguous
            and rng_states.size % 6 == 0):
        raise ValueError('rng_states: a contiguous uint32 array of 6*nslots words')
    ngen, exhausted = ctypes.c_uint32(), ctypes.c_uint32()
    _native.call('chr_generate_photons_host', ctypes.byref(packed.desc()), rec.ctypes.data, len(rec),
                 ctypes.byref(desc), int(first_photon), cap, rng_states.ctypes.data, rng_states.size // 6,
                 ctypes.byref(ngen), ctypes.byref(exhausted))
    assert ngen.value == n
    return event.Photons(arrays['pos'], arrays['dir'], arrays['pol'], arrays['wavelengths'], arrays['t'],
                         arrays['last_hit_triangles'], arrays['flags'], arrays['weights'], arrays['evidx']), \
        exhausted.value
