"""Step cache: skip the MMDiT blocks on denoise steps whose input barely moved (TeaCache, Liu et al. 2024).

Host logic only -- no tensors live here.  The pipeline measures, per step, how far the first block's modulated image input
moved since the previous step (``ops.absdiff_sums``: sum |cur - prev| and sum |prev|), hands the two sums to
:meth:`StepCache.step`, and gets back whether the step runs the blocks or adds the residual (block output minus block input)
kept at the last computed step.

Two modes, exactly one of which must be chosen:

``threshold=``  adaptive.  Step 0 and the last executed step always compute.  At step ``i >= 1``:
                ``rel = sums[0] / sums[1]`` (inf when the denominator is 0), ``acc += polyval(coefficients, rel)``,
                the step computes when ``acc >= threshold``, and ``acc`` returns to 0 after a computed step.
                ``coefficients`` (lowest order first) defaults to the identity: the rescaling polynomial TeaCache publishes
                for FLUX was fitted to another checkpoint, so it is a parameter here, and there is no default threshold.
``schedule=``   an iterable of executed-step indices that compute (index 0 = the first step actually run, i.e. ``t_start``
                when ``strength < 1``).  Must contain 0, be strictly increasing and lie inside the step count.  Nothing is
                measured and nothing is read back: the loop stays sync-free and graph-capturable.

``measure="first_block"`` (the first-block cache of ParaAttention / diffusers' ``FirstBlockCacheConfig``) changes what
is measured and what is skipped.  Block 0 runs at EVERY step; ``r1`` is what it added to the image stream.  Adaptive:
``rel = sum|r1 - ref| / sum|ref|`` against the ``r1`` of the last computed step (``ops.residual_absdiff_sums``), and the step
computes iff ``rel >= threshold`` -- nothing is accumulated (``ref`` stays put, so drift adds up by itself) and there is no
polynomial (``coefficients`` other than the default is a ``ValueError``).  A skipped step adds the residual of blocks 1 .. end
kept at the last computed step to block 0's output.  ``schedule=`` names the same steps with nothing measured.

After a call ``computed_steps`` lists the computed step indices, ``block_passes`` counts the passes through the blocks the
transformer made and, in adaptive mode, ``rel_l1`` holds the per-step floats (steps 1 .. n-1); ``StepCache(schedule=sc.computed_steps)`` replays an adaptive run's decisions.
"""
import math


MEASURES = ("input", "first_block")


class StepCache:
    def __init__(self, threshold=None, schedule=None, coefficients=(0.0, 1.0), measure="input"):
        if measure not in MEASURES:
            raise ValueError(f"`measure` must be one of {MEASURES}, got {measure!r}")
        self.measure = measure
        if (threshold is None) == (schedule is None):
            raise ValueError("StepCache takes exactly one of `threshold` (adaptive) and `schedule` (fixed)")
        self.threshold = None
        self.schedule = None
        if threshold is not None:
            self.threshold = float(threshold)
            if math.isnan(self.threshold) or self.threshold < 0:
                raise ValueError(f"`threshold` must be a number >= 0, got {threshold!r}")
        else:
            raw = list(schedule)
            sched = [int(i) for i in raw]
            if any(i != j for i, j in zip(sched, raw)):
                raise ValueError(f"`schedule` holds step indices (integers), got {raw!r}")
            if not sched or sched[0] != 0:
                raise ValueError("`schedule` must contain step 0: the first executed step has no residual to reuse")
            if any(b <= a for a, b in zip(sched, sched[1:])):
                raise ValueError(f"`schedule` must be strictly increasing, got {sched}")
            self.schedule = tuple(sched)
        self.coefficients = tuple(float(c) for c in coefficients)
        if not self.coefficients:
            raise ValueError("`coefficients` must hold at least one value (lowest order first)")
        if self.first_block and self.coefficients != (0.0, 1.0):
            raise ValueError('`coefficients` belongs to measure="input": the first-block measure is a plain relative change')
        self.begin(0)

    @property
    def adaptive(self):
        return self.threshold is not None

    @property
    def first_block(self):
        return self.measure == "first_block"

    # ---- pure pieces -------------------------------------------------------------------------------------------------
    @staticmethod
    def polyval(coefficients, x):
        """c0 + c1 x + c2 x^2 + ... (lowest order first), Horner's scheme in Python floats."""
        y = 0.0
        for c in reversed(tuple(coefficients)):
            y = y * x + c
        return y

    @staticmethod
    def rel_of(sums):
        """sums = (sum |cur - prev|, sum |prev|) -> their ratio as a Python float; a zero denominator gives inf."""
        num, den = float(sums[0]), float(sums[1])
        return math.inf if den == 0.0 else num / den

    def decide(self, acc, rel, i, n):
        """(compute, acc after the step) of executed step ``i`` of ``n``: the whole adaptive rule, a pure function of its
        arguments and the constructor's ``threshold`` / ``coefficients``.  ``rel`` is ignored at step 0 (nothing to compare
        with); the first and the last step compute whatever the measure says."""
        if i == 0:
            return True, 0.0
        if self.first_block:         # no accumulation: the reference residual stays where it is, so drift adds up by itself
            return i == n - 1 or math.isnan(rel) or rel >= self.threshold, 0.0
        acc = acc + self.polyval(self.coefficients, rel)
        if math.isnan(acc):          # inf - inf through a polynomial with a negative coefficient: never skip on a NaN
            acc = math.inf
        compute = i == n - 1 or acc >= self.threshold
        return compute, (0.0 if compute else acc)

    def validate(self, n):
        """Raise ``ValueError`` when the schedule does not fit ``n`` executed steps (called before any GPU work)."""
        if n < 1:
            raise ValueError("a step cache needs at least one executed step")
        if self.schedule is not None and self.schedule[-1] >= n:
            raise ValueError(f"`schedule` names step {self.schedule[-1]}, the call executes steps 0 .. {n - 1}")

    # ---- per call ----------------------------------------------------------------------------------------------------
    def begin(self, n):
        """Start a call of ``n`` executed steps: clears the records."""
        self._n = int(n)
        self._acc = 0.0
        self.computed_steps = []
        self.rel_l1 = []
        self.block_passes = 0         # set by the pipeline: passes through the blocks the call made (state.block_passes)

    def scheduled(self, i):
        return i in self.schedule

    def step(self, i, sums=None):
        """Decide executed step ``i``.  Adaptive mode takes the step's two sums (any pair ``float()`` accepts; ignored at step
        0); schedule mode takes nothing."""
        if self.adaptive:
            rel = 0.0
            if i > 0:
                rel = self.rel_of(sums)
                self.rel_l1.append(rel)
            compute, self._acc = self.decide(self._acc, rel, i, self._n)
        else:
            compute = self.scheduled(i)
        if compute:
            self.computed_steps.append(i)
        return compute


def parse_int_list(text):
    """'0,1,3' -> [0, 1, 3] (command-line form of ``schedule``)."""
    return [int(p) for p in str(text).split(",") if p.strip() != ""]


def parse_float_list(text):
    """'0.0,1.0' -> [0.0, 1.0] (command-line form of ``coefficients``)."""
    return [float(p) for p in str(text).split(",") if p.strip() != ""]


def from_args(threshold=None, schedule=None, coefficients=None, measure=None):
    """The command line's four options -> a StepCache, or None when neither mode is asked for."""
    if threshold is None and schedule is None:
        if coefficients is not None:
            raise ValueError("--step_cache_coefficients needs --step_cache_threshold")
        return None
    kw = {}
    if measure is not None:
        kw["measure"] = measure
    if coefficients is not None:
        kw["coefficients"] = parse_float_list(coefficients)
    return StepCache(threshold=threshold, schedule=None if schedule is None else parse_int_list(schedule), **kw)
