"""The logits lens of the end-to-end tests: all `ncls` logits of every mask row against the fp64 restatement, not one softmax probability.

A softmax score cancels an error common to a row's logits and hides errors on classes of low probability; the logits show both.  The
yardstick is reference against reference: d_L = max |fp32 batch-1 CPU loop logits - fp64 logits| over all rows and classes a test feeds
in.  The bound on |engine - fp64| is 4 d_L: the engine stores every activation as hi + lo, 22 bits, four fp32 roundings, and 4 is the
factor the end-to-end score rule already uses.  Nothing here is taken from the engine's own output."""
import numpy as np

FACTOR = 4.0


class LogitsLens:
    def __init__(self, name):
        self.name = name
        self.d_loop = 0.0           # fp32 batch-1 CPU loop against fp64: the yardstick
        self.d_engine = 0.0         # the engine against fp64
        self.rows = 0

    def add(self, what, engine_logits, loop_logits, logits64):
        """One case: engine f32[M, ncls], fp32 CPU loop f32[M, ncls], fp64 [M, ncls]."""
        logits64 = np.asarray(logits64, dtype=np.float64)
        assert engine_logits.shape == loop_logits.shape == logits64.shape and logits64.ndim == 2, (engine_logits.shape, loop_logits.shape, logits64.shape)
        assert np.isfinite(engine_logits).all() and np.isfinite(logits64).all()
        d_loop = float(np.abs(loop_logits.astype(np.float64) - logits64).max())
        d_engine = float(np.abs(engine_logits.astype(np.float64) - logits64).max())
        print("%s %s logits: %d rows x %d classes, |logit| up to %.2f, fp32 CPU loop vs fp64 %.3e, engine vs fp64 %.3e"
              % (self.name, what, logits64.shape[0], logits64.shape[1], np.abs(logits64).max(), d_loop, d_engine))
        self.d_loop = max(self.d_loop, d_loop)
        self.d_engine = max(self.d_engine, d_engine)
        self.rows += logits64.shape[0]

    def check(self):
        assert self.rows > 0 and self.d_loop > 0.0
        ratio = self.d_engine / self.d_loop
        print("%s logits lens over %d rows: d_L %.3e, engine %.3e, engine / d_L %.2f (bound %.0f)" % (self.name, self.rows, self.d_loop, self.d_engine, ratio, FACTOR))
        assert self.d_engine <= FACTOR * self.d_loop, (self.name, self.d_engine, self.d_loop, ratio)
        return self.d_loop, self.d_engine
