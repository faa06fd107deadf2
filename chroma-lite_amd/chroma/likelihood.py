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
