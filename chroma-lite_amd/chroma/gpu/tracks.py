"""PhotonTracks: the tracks of one tracked propagate, recorded on the device
(chr_propagate_tracked; replaces the per-step copy_queue and downloads of the
reference's GPUPhotons.propagate(track=True), photon.py:252-293).

A track record is 16 u32 words (CHR_TRACK_WORDS, include/chroma_amd.h):
[0] photon id, [1] history, [2:5] pos, [5:8] dir, [8:11] pol, [11] wavelength,
[12] t, [13] weight, [14] last-hit triangle, [15] entry index.  The handle holds
them in two orders: step-major (entry 0 = the input state of the first queue,
entry k = the queue of step k after k steps; offsets per entry) and
photon-major (each photon's records by entry; offsets per photon).  evidx is not
recorded: it is the photons' evidx gathered by id.
"""
import ctypes

import numpy as np

from chroma import event
from chroma.gpu import _native

TRACK_WORDS = 16
STEP_MAJOR, PHOTON_MAJOR = 0, 1


def unpack_records(records, evidx):
    """(ids uint32, event.Photons) of an (n, 16) uint32 record array, record r at
    element r: one native pass over the records (chr_tracks_unpack).  evidx: the
    propagate's evidx array (all copies), gathered by the records' ids."""
    rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, TRACK_WORDS)
    evidx = np.ascontiguousarray(evidx, dtype=np.uint32)
    n = len(rec)
    f32, u32 = np.float32, np.uint32
    out = dict(pos=np.empty((n, 3), f32), dir=np.empty((n, 3), f32), pol=np.empty((n, 3), f32),
               wavelengths=np.empty(n, f32), t=np.empty(n, f32), weights=np.empty(n, f32), flags=np.empty(n, u32),
               last_hit_triangles=np.empty(n, np.int32), evidx=np.empty(n, u32))
    ids = np.empty(n, u32)
    desc = _native.PhotonsDesc(*[out[f].ctypes.data for f in ('pos', 'dir', 'pol', 'wavelengths', 't', 'weights',
                                                              'flags', 'last_hit_triangles', 'evidx')])
    _native.call('chr_tracks_unpack', rec.ctypes.data, n, evidx.ctypes.data, len(evidx), ctypes.byref(desc),
                 ids.ctypes.data)
    return ids, event.Photons(out['pos'], out['dir'], out['pol'], out['wavelengths'], out['t'],
                              out['last_hit_triangles'], out['flags'], out['weights'], out['evidx'])


def photons_from_records(records, evidx):
    """event.Photons of an (n, 16) uint32 record array."""
    return unpack_records(records, evidx)[1]


def steps_from_records(records, counts, evidx):
    """(step_photon_ids, step_photons) of step-major records: per entry the ids
    (uint32) and the photons, what the reference's track=True returns (slices
    of one set of arrays that holds every entry back to back)."""
    bounds = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]).tolist()
    ids, photons = unpack_records(records, evidx)
    if bounds[-1] != len(ids):
        raise ValueError('%d records for entries of %d in all' % (len(ids), bounds[-1]))
    return ([ids[a:b] for a, b in zip(bounds[:-1], bounds[1:])],
            [photons[a:b] for a, b in zip(bounds[:-1], bounds[1:])])


class _DeviceWords(object):
    """A device buffer of the handle as torch sees it (__cuda_array_interface__);
    it keeps the PhotonTracks, and so the handle, alive."""

    def __init__(self, owner, ptr, nwords, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = dict(shape=(int(nwords),), typestr=typestr, data=(int(ptr), False), version=2,
                                             strides=None)


class PhotonTracks(object):
    def __init__(self, handle, evidx, nphotons=None):
        """handle: the chr_tracks* of chr_propagate_tracked (owned from here on);
        evidx: the photons' evidx, a GPUArray (downloaded on first host use) or
        a host array."""
        self._handle = ctypes.c_void_p(handle) if not isinstance(handle, ctypes.c_void_p) else handle
        self._evidx = evidx
        self._host = {}
        self.last_stats = None
        ne, nr, nph = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32()
        _native.call('chr_tracks_info', self._handle, ctypes.byref(ne), ctypes.byref(nr), ctypes.byref(nph))
        self.nentries, self.nrecords, self.nphotons = int(ne.value), int(nr.value), int(nph.value)
        counts = np.zeros(max(self.nentries, 1), dtype=np.uint64)
        _native.call('chr_tracks_entry_counts', self._handle, counts.ctypes.data)
        self.step_counts = counts[:self.nentries].astype(np.int64)

    # ------------------------------------------------------------ the seam of the CPU tests
    @classmethod
    def from_host(cls, step_records, step_counts, evidx, nphotons, flat_records=None, flat_offsets=None):
        """A PhotonTracks over host buffers (no handle, no device): what the
        downloads of a handle would give.  The photon-major order is derived
        from the step-major records when it is not given."""
        self = cls.__new__(cls)
        self._handle = None
        self._evidx = np.asarray(evidx, dtype=np.uint32)
        rec = np.ascontiguousarray(step_records, dtype=np.uint32).reshape(-1, TRACK_WORDS)
        self.step_counts = np.asarray(step_counts, dtype=np.int64)
        self.nentries, self.nrecords, self.nphotons = len(self.step_counts), len(rec), int(nphotons)
        self.last_stats = None
        if flat_records is None:
            flat_offsets = np.concatenate([[0], np.cumsum(np.bincount(rec[:, 0], minlength=self.nphotons))])
            flat_records = rec[np.lexsort((rec[:, 15], rec[:, 0]))]
        soff = np.concatenate([[0], np.cumsum(self.step_counts)]).astype(np.uint64)
        self._host = {STEP_MAJOR: (rec, soff),
                      PHOTON_MAJOR: (np.ascontiguousarray(flat_records, dtype=np.uint32).reshape(-1, TRACK_WORDS),
                                     np.asarray(flat_offsets, dtype=np.uint64))}
        return self

    # ------------------------------------------------------------ lifetime
    def close(self):
        """Free the device buffers (chr_tracks_free); host copies already made stay."""
        h, self._handle = getattr(self, '_handle', None), None
        if h is not None and h.value:
            _native.lib().chr_tracks_free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------ downloads
    def _evidx_host(self):
        if not isinstance(self._evidx, np.ndarray):
            self._evidx = self._evidx.get()
        return self._evidx

    def records(self, order=STEP_MAJOR):
        """(records (nrecords, 16) uint32, offsets uint64) of one order: one
        download (chr_tracks_copy), kept on the host afterwards."""
        if order not in self._host:
            if self._handle is None:
                raise ValueError('the tracks are closed')
            rec = np.empty((self.nrecords, TRACK_WORDS), dtype=np.uint32)
            off = np.zeros((self.nphotons if order == PHOTON_MAJOR else self.nentries) + 1, dtype=np.uint64)
            _native.call('chr_tracks_copy', self._handle, int(order), rec.ctypes.data, off.ctypes.data)
            self._host[order] = (rec, off)
        return self._host[order]

    def steps(self):
        """(step_photon_ids, step_photons): per entry the uint32 ids and the
        event.Photons, as the reference's propagate(track=True) returns them."""
        rec, _ = self.records(STEP_MAJOR)
        return steps_from_records(rec, self.step_counts, self._evidx_host())

    def flat(self):
        """(offsets, photons): photon i's track is photons[offsets[i]:offsets[i + 1]],
        its j-th record the state after j steps (offsets: int64, nphotons + 1)."""
        if 'flat' not in self._host:
            rec, off = self.records(PHOTON_MAJOR)
            self._host['flat'] = (off.astype(np.int64), photons_from_records(rec, self._evidx_host()))
        return self._host['flat']

    def track(self, i):
        """The track of photon i as event.Photons (entry 0 first)."""
        off, photons = self.flat()
        if not 0 <= i < self.nphotons:
            raise IndexError('photon %d of %d' % (i, self.nphotons))
        return photons[int(off[i]):int(off[i + 1])]

    def __len__(self):
        return self.nphotons

    def device(self, order=STEP_MAJOR):
        """(records, offsets) of one order where they are: GPUArrays (uint32,
        nrecords * 16 words; uint64) that are views of the handle's buffers and
        keep it alive."""
        import torch
        from chroma.gpu import gpuarray as ga
        if self._handle is None:
            raise ValueError('the tracks are closed or were made on the host')
        d_rec, d_off = ctypes.c_void_p(), ctypes.c_void_p()
        _native.call('chr_tracks_device', self._handle, int(order), ctypes.byref(d_rec), ctypes.byref(d_off))
        noff = (self.nphotons if order == PHOTON_MAJOR else self.nentries) + 1

        def view(ptr, nwords, typestr, dtype, torch_dtype):
            if not ptr or nwords == 0:
                return ga.zeros(nwords, dtype)
            t = torch.as_tensor(_DeviceWords(self, ptr, nwords, typestr), device=ga._device())
            assert t.dtype == torch_dtype and t.data_ptr() == ptr
            return ga.GPUArray((nwords,), dtype, t)
        return (view(d_rec.value, self.nrecords * TRACK_WORDS, '<i4', np.uint32, torch.int32),
                view(d_off.value, noff, '<i8', np.uint64, torch.int64))
