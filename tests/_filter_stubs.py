"""Stand-in filters on the CPU for the tests of ``evaluation.run_filter``, which is duck-typed: fixed estimates in place of
a run, and a log of what was called with which arguments and under which ``record_*`` switches.  Shared by
``test_run_filter_cpu.py``, ``test_density_cases_cpu.py`` and ``test_mode_cases_cpu.py``."""
SWITCHES = ("record_belief", "record_history", "record_innovations", "record_transition_moments")


class _Recorded:
    """``forward_loop`` returns fixed estimates; with a covariance it keeps a belief record like a Kalman filter, without one
    it is a point estimator like the LSTM baselines."""

    def __init__(self, est, cov=None):
        self._est, self._cov = est, cov
        if cov is not None:
            self.record_belief, self.last_belief = False, None

    def initialize_beliefs(self, *, mean, covariance):
        pass

    def forward_loop(self, *, observations, controls):
        if self._cov is not None:
            from multimodalfilter_amd import base

            self.last_belief = base.belief_record(covariance=self._cov) if self.record_belief else None
        return self._est


class _Logged:
    """A filter with ``record_belief``, ``record_history``, ``forward_loop`` and ``smooth`` that returns the fixed ``est`` and
    ``smoothed`` under the fixed covariances.  ``calls``: ``(name, arguments, switches)`` of every call, ``switches`` the
    ``record_*`` attributes as they stood then.  ``fail``: the name of the method that raises ``RuntimeError``."""

    def __init__(self, est, cov, smoothed, smoothed_cov, prior=False):
        self._est, self._cov, self._smoothed, self._smoothed_cov = est, cov, smoothed, smoothed_cov
        self.record_belief = self.record_history = prior
        self.last_belief = self.last_history = self.last_smoothed = None
        self.calls, self.fail = [], None

    def switches(self):
        return {k: getattr(self, k) for k in SWITCHES if hasattr(self, k)}

    def _log(self, name, **arguments):
        self.calls.append((name, arguments, self.switches()))
        if self.fail == name:
            raise RuntimeError(f"{name} fails")

    def called(self, name):
        return [c for c in self.calls if c[0] == name]

    def initialize_beliefs(self, *, mean, covariance):
        self._log("initialize_beliefs")

    def forward_loop(self, *, observations, controls):
        from multimodalfilter_amd import base

        self._log("forward_loop")
        self.last_belief = base.belief_record(covariance=self._cov) if self.record_belief else None
        self.last_history = object() if self.record_history else None
        return self._est

    def smooth(self, lag=None, *, method="ancestry", **more):
        from multimodalfilter_amd import base

        self._log("smooth", lag=lag, method=method, **more)
        self.last_smoothed = base.belief_record(covariance=self._smoothed_cov, method=method)
        return self._smoothed


class _Kalman(_Logged):
    """... with ``record_innovations`` as well: the Kalman filters' side of ``run_filter``."""

    def __init__(self, *args, prior=False):
        super().__init__(*args, prior=prior)
        self.record_innovations, self.last_innovations = prior, None

    def forward_loop(self, *, observations, controls):
        self.last_innovations = object() if self.record_innovations else None
        return super().forward_loop(observations=observations, controls=controls)


class _Particles(_Logged):
    """... with the ``belief_*`` methods of ``ParticleFilter``, each of which logs its arguments and leaves a new ``last_*``
    object.  ``crossmodal``: the measurement model is a ``CrossmodalParticleFilterMeasurementModel`` (never called) and the
    filter has ``record_transition_moments``; without it the filter is a particle filter that fuses nothing and computes no
    transition moments."""

    def __init__(self, *args, prior=False, crossmodal=True):
        super().__init__(*args, prior=prior)
        self.last_scores = self.last_density = self.last_modes = self.last_modalities = self.last_quantiles = None
        self.measurement_model = None
        if crossmodal:
            from multimodalfilter_amd.base_models import CrossmodalParticleFilterMeasurementModel

            self.measurement_model = object.__new__(CrossmodalParticleFilterMeasurementModel)
            self.record_transition_moments = prior

    def belief_scores(self, truth, *, of="filtered", scale=None):
        self._log("belief_scores", truth=truth, of=of, scale=scale)
        self.last_scores = object()

    def belief_density(self, truth=None, *, of="filtered", bandwidth="silverman"):
        self._log("belief_density", truth=truth, of=of, bandwidth=bandwidth)
        self.last_density = object()

    def belief_modes(self, of="filtered", *, max_modes=4, link_radius=3.0):
        self._log("belief_modes", of=of, max_modes=max_modes, link_radius=link_radius)
        self.last_modes = object()

    def belief_modalities(self):
        self._log("belief_modalities")
        self.last_modalities = object()

    def belief_quantiles(self, probs, *, of="filtered", truth=None):
        self._log("belief_quantiles", probs=probs, of=of, truth=truth)
        self.last_quantiles = object()
