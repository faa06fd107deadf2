"""Negative log likelihood of an observed detector event given photon sources
(the callers' side of reference chroma/likelihood.py), over
Simulation.eval_pdf / setup_kernel / eval_kernel.

A likelihood point simulates `nevals` sources, each propagated `nreps` times
and each propagated copy read out by `ndaq` DAQ copies: ntotal = nevals *
nreps * ndaq trials per channel.  From them come, per channel, the probability
of a hit (hits / ntotal) and the density of the observed time at the hit
channels.  `uncertainties` is not a dependency here: eval returns a float
(its uncertainty is identically 0 in the reference), eval_kernel returns
(mean, standard error).
"""
from itertools import islice
from math import sqrt

import numpy as np

from chroma.log import logger


class Likelihood(object):
    """Likelihoods of one detector event (an event.Event with channels)."""

    def __init__(self, sim, event=None, tbins=100, trange=(-0.5, 999.5), qbins=10, qrange=(-0.5, 49.5),
                 time_only=True):
        """sim: the chroma.sim.Simulation that propagates the sources; event: the
        observed event (or set_event later); trange / qrange: the time and
        charge windows of the PDFs; tbins / qbins: kept for histogram PDFs
        (Simulation.create_pdf); time_only: the density is over time alone."""
        self.sim = sim
        self.tbins, self.trange, self.qbins, self.qrange = tbins, trange, qbins, qrange
        self.time_only = time_only
        self.event = None
        if event is not None:
            self.set_event(event)

    def set_event(self, event):
        """The observed event to evaluate."""
        self.event = event

    # ------------------------------------------------------------ pieces
    def flat_density(self):
        """The density of an observable spread evenly over the PDF's range: what a
        channel without usable simulated data is given."""
        flat = 1.0 / (self.trange[1] - self.trange[0])
        if not self.time_only:
            flat /= self.qrange[1] - self.qrange[0]
        return flat

    def _floor_densities(self, value, uncert):
        """Non-positive and NaN densities (and their uncertainties) -> flat_density()."""
        unusable = np.isnan(value) | (value <= 0.0)
        value[unusable] = self.flat_density()
        uncert[unusable] = self.flat_density()
        logger.info('channels with no data: %d', int(np.count_nonzero(unusable & self.event.channels.hit)))
        return value, uncert

    def eval_channel_vbin(self, sources, nevals, nreps=16, ndaq=50):
        """(hit probability, PDF value, PDF uncertainty) per channel from the first
        `nevals` of `sources`, by the adaptive-bin method (Simulation.eval_pdf:
        bins of 0.2 in time and 1 in charge, widened to hold 320 entries)."""
        ntotal = nevals * nreps * ndaq
        hitcount, value, uncert = self.sim.eval_pdf(self.event.channels, islice(sources, nevals), 0.2, self.trange,
                                                    1, self.qrange, min_bin_content=320, nreps=nreps, ndaq=ndaq,
                                                    time_only=self.time_only)
        value, uncert = self._floor_densities(np.array(value, dtype=float), np.array(uncert, dtype=float))
        return hitcount.astype(np.float32) / ntotal, value, uncert

    def eval(self, sources, nevals, nreps=16, ndaq=50):
        """-log L of the event given `sources`: over all channels the probability
        of what the channel did (hit or not, floored at half a trial), times
        the density of the observed time at the hit channels."""
        ntotal = nevals * nreps * ndaq
        hit_prob, value, _ = self.eval_channel_vbin(sources, nevals, nreps, ndaq)
        observed = np.asarray(self.event.channels.hit, dtype=bool)
        prob = np.where(observed, hit_prob, 1.0 - hit_prob)
        prob = np.maximum(prob, 0.5 / ntotal)
        return -float(np.log(prob).sum() + np.log(value[observed]).sum())

    # ------------------------------------------------------------ kernel estimator
    def setup_kernel(self, sources, nevals, nreps, ndaq, oversample_factor):
        """Choose the kernel bandwidths from nevals * oversample_factor sources."""
        self.sim.setup_kernel(self.event.channels, islice(sources, nevals * oversample_factor), self.trange,
                              self.qrange, nreps=nreps, ndaq=ndaq, time_only=self.time_only,
                              scale_factor=oversample_factor)

    def eval_kernel(self, sources, nevals, nreps=16, ndaq=50, navg=10):
        """(mean, standard error) of -log L over `navg` kernel estimates of nevals
        sources each, after setup_kernel.  Only the densities at the hit
        channels enter (the reference leaves the hit probabilities out of this
        estimate); estimates that are not finite are left out."""
        observed = np.asarray(self.event.channels.hit, dtype=bool)
        logs = []
        for _ in range(navg):
            _, value, uncert = self.sim.eval_kernel(self.event.channels, islice(sources, nevals), self.trange,
                                                    self.qrange, nreps=nreps, ndaq=ndaq, time_only=self.time_only)
            value, _ = self._floor_densities(np.array(value, dtype=float), np.array(uncert, dtype=float))
            ll = float(np.log(value[observed]).sum())
            logger.debug('kernel estimate: log likelihood %g', ll)
            if np.isfinite(ll):
                logs.append(ll)
        if not logs:
            raise ValueError('no finite kernel estimate in %d tries' % navg)
        logs = np.array(logs)
        mean = logs.mean()
        rms = sqrt(max(0.0, float((logs ** 2).mean() - mean ** 2)))
        return -float(mean), rms / sqrt(len(logs))


class LibraryLikelihood(object):
    """Negative log likelihood of one observed event from a photon library
    (chroma.gpu.GPUPhotonLibrary or HostPhotonLibrary), without propagating a
    photon: library.log_likelihood (chr_library_loglike; the rule is written out in
    include/chroma_amd.h) scores many hypotheses in one call.

    -log L is a sum over the channels of a charge term -- Poisson in the observed
    photo-electron count, or hit / no hit -- and, at the hit channels of a library
    with a time histogram, the density of the observed time under "library signal
    plus flat noise".  What to know about the numbers:
      * the Poisson form leaves out lgamma(n + 1): it is the same for every
        hypothesis, so differences and minima of -log L are unaffected, the value is not
        a normalised likelihood;
      * a channel's term is clamped to +-2^23 (an observed hit where the hypothesis
        and the floor expect nothing costs 2^23, not infinity) and kept in units of
        2^-20, so values are exact sums, independent of how the device adds them;
      * `bad` (of the last call, self.last) counts the channels whose term was a NaN
        (an infinite expectation) and entered as 0; `skipped` the entries whose
        source the library does not have."""

    # bytes of the entry table of one call: a one-entry hypothesis takes 20 (an
    # offset, a source, a photon count, a time); scan() and best() split at this,
    # and at the hypotheses one call accepts: hypotheses x nchannels <= 2^31, the
    # limit log_likelihood inherits from expect (74,033 on 29,007 channels)
    group_bytes = 64 << 20

    def __init__(self, library, channels_or_sampled, mode='poisson', floor=1e-3, use_times=True, tfloor=None):
        """channels_or_sampled: an event.Channels (hit mode: n = hit; Poisson mode:
        n = rint(q), negatives and NaN to 0; t is taken at the hit channels only),
        or a pair (n, t) of numpy or device arrays used as they are (t may be None),
        or a one-event Sampled, whose device n and t are used without a download.
        use_times: use t when the library keeps a time histogram."""
        self.library, self.mode, self.floor, self.tfloor = library, mode, floor, tfloor
        self.n, t = self.observed(channels_or_sampled, mode)
        self.t = t if (use_times and t is not None and library.tbins > 0) else None
        self.last = None

    @staticmethod
    def observed(channels_or_sampled, mode='poisson'):
        """(n, t) of what LibraryLikelihood is given (see __init__)."""
        c = channels_or_sampled
        if isinstance(c, (tuple, list)):
            n, t = c
            return n, t
        if hasattr(c, 'n') and hasattr(c, 'nevents'):                   # a Sampled
            if c.nevents != 1:
                raise ValueError('a Sampled of %d events: one observed event is scored at a time' % c.nevents)
            return c.n, c.t
        hit = np.asarray(c.hit, dtype=bool)
        if mode == 'hit':
            n = hit.astype(np.uint32)
        else:
            q = np.nan_to_num(np.asarray(c.q, np.float64), nan=0.0, posinf=2.0 ** 32 - 1, neginf=0.0)
            n = np.clip(np.rint(q), 0, 2.0 ** 32 - 1).astype(np.uint32)
        t = np.where(hit, np.asarray(c.t, np.float32), np.float32(np.nan)).astype(np.float32)
        return n, t

    def eval(self, entries):
        """-log L (float64) of every hypothesis of a chroma.library.LibraryEntries."""
        self.last = self.library.log_likelihood(entries, self.n, self.t, mode=self.mode, floor=self.floor,
                                                tfloor=self.tfloor).get()
        return -self.last.ll

    def _eval_single(self, source, nphotons, t0):
        """-log L of the one-entry hypotheses (source[k], nphotons[k], t0[k]), in groups
        whose entry tables stay under group_bytes and whose hypotheses x nchannels
        stay within the 2^31 a call accepts."""
        from chroma.library import LibraryEntries
        from chroma.library import MAX_WORDS
        out = np.empty(len(source), np.float64)
        per = max(1, min(int(self.group_bytes) // 20, MAX_WORDS // int(self.library.nchannels)))
        for k in range(0, len(source), per):
            m = len(source[k:k + per])
            out[k:k + m] = self.eval(LibraryEntries(np.arange(m + 1), source[k:k + m], nphotons[k:k + m],
                                                    t0[k:k + m]))
        return out

    def scan(self, nphotons, t0=0.0):
        """-log L of "nphotons photons made at t0 in voxel s" for every source s of the
        library: nsources values, as an array of the library's VoxelGrid's shape
        (indexed [ix, iy, iz]) when it has one."""
        ns = self.library.nsources
        out = self._eval_single(np.arange(ns), np.full(ns, nphotons, np.int64), np.full(ns, t0, np.float32))
        grid = self.library.grid
        return out if grid is None else out.reshape(grid.shape, order='F')

    def best(self, nphotons_list, t0_list):
        """(voxel, nphotons, t0, -log L) of the smallest -log L over every source x
        nphotons_list x t0_list (the first one in that order -- nphotons slowest, the
        voxel fastest -- when several tie)."""
        ns = self.library.nsources
        nph, t0s = np.asarray(nphotons_list, np.int64).reshape(-1), np.asarray(t0_list, np.float32).reshape(-1)
        if not (len(nph) and len(t0s)):
            raise ValueError('best() needs at least one photon count and one time')
        ip, it, s = np.unravel_index(np.arange(len(nph) * len(t0s) * ns), (len(nph), len(t0s), ns))
        nll = self._eval_single(s, nph[ip], t0s[it])
        k = int(np.argmin(nll))
        return int(s[k]), int(nph[ip[k]]), float(t0s[it[k]]), float(nll[k])
