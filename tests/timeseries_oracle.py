"""Long-double restatement of the timeseries quantities (CPU, numpy only): suffix means, centered lag sums and the stopping rule of
the statistical inefficiency.  Written from the definitions, not from any implementation.

* :func:`centered_sum` is the exact oracle of one (origin, lag) pair: the sum about the suffix means, formed term by term in long
  double.  The GPU tests check the device against it.
* :class:`OracleACF` is a CPU stand-in for ``pymbar_amd.timeseries.DeviceACF`` with the same methods (vectorised over origins
  with long-double suffix sums), so that the whole public module runs without a device.
"""
import numpy as np

LD = np.longdouble
STOPPED, ZERO_VARIANCE, END = 1, 2, 3


def centered_sum(a, b, s, t):
    """sum_{n=s}^{T-1-t} (a_n - mean(a[s:])) (b_(n+t) - mean(b[s:])) in long double (b None: a)."""
    a = np.asarray(a, dtype=LD)
    b = a if b is None else np.asarray(b, dtype=LD)
    T = a.size
    if t >= T - s:
        return LD(0)
    ma, mb = a[s:].sum() / LD(T - s), b[s:].sum() / LD(T - s)
    return np.sum((a[s:T - t] - ma) * (b[s + t:] - mb))


def rule_trace(a, s, fast, mintime, fft=False, b=None):
    """The stopping rule at origin s, term by term in long double: (g, stop, status, [(t, C), ...] evaluated)."""
    T = len(a)
    N = T - s
    sig2 = centered_sum(a, b, s, 0) / LD(N)
    if sig2 == 0:
        return 1.0, 0, ZERO_VARIANCE, []
    g = LD(1)
    t, inc, trace = 1, 1, []
    tend = N if fft else N - 1
    while t < tend:
        x = centered_sum(a, b, s, t)
        if b is not None:
            x = x + centered_sum(b, a, s, t)
        else:
            x = 2 * x
        C = x / (2 * LD(N - t) * sig2)
        trace.append((t, C))
        if C <= 0 and t > mintime:
            return max(float(g), 1.0), t, STOPPED, trace
        g += 2 * C * (1 - LD(t) / LD(N)) * inc
        t += inc
        if fast:
            inc += 1
    return max(float(g), 1.0), t, END, trace


def _schedule(fast, tmax):
    out, t, inc = [], 1, 1
    while t < tmax:
        out.append((t, inc))
        t += inc
        if fast:
            inc += 1
    return out


class OracleACF:
    """CPU stand-in of DeviceACF: same constructor and methods, long-double sums."""

    def __init__(self, a, b=None, seg=None, shift_a=0.0, shift_b=0.0, device=None):
        self.a = np.asarray(a, dtype=LD)
        self.b = None if b is None else np.asarray(b, dtype=LD)
        self.T = self.a.size
        self.seg = np.asarray([self.T] if seg is None else seg, dtype=np.int64)
        self.shift_a, self.shift_b = LD(shift_a), LD(shift_b)
        ends = np.cumsum(self.seg)
        self.rem = np.repeat(ends, self.seg) - np.arange(self.T)  # positions left in each value's segment
        if not (np.all(np.isfinite(self.a)) and (self.b is None or np.all(np.isfinite(self.b)))):
            raise ValueError("the series must be finite")

    def _bb(self):
        return self.a if self.b is None else self.b

    def _suffix_x(self, t, x, y):
        """per origin s: sum_{n >= s, n + t valid} x_n y_(n+t), x and y about their suffix means (one segment)."""
        T = self.T
        mx = np.cumsum(x[::-1])[::-1] / np.arange(T, 0, -1).astype(LD)
        my = np.cumsum(y[::-1])[::-1] / np.arange(T, 0, -1).astype(LD)
        out = np.zeros(T, dtype=LD)
        if t >= T:
            return out
        # sum (x_n - mx_s)(y_(n+t) - my_s) = Sxy - my_s Sx - mx_s Sy + (N - t) mx_s my_s over n in [s, T - t)
        pxy = np.concatenate([np.cumsum((x[:T - t] * y[t:])[::-1])[::-1], np.zeros(t + 1, LD)])
        sx = np.concatenate([np.cumsum(x[::-1])[::-1], [LD(0)]])
        sy = np.concatenate([np.cumsum(y[::-1])[::-1], [LD(0)]])
        s = np.arange(T)
        cnt = np.maximum(T - s - t, 0).astype(LD)
        lo = np.minimum(s, T - t)
        Sx = sx[lo] - sx[T - t]
        Sy = sy[np.minimum(s + t, T)]
        out = pxy[lo] - my * Sx - mx * Sy + cnt * mx * my
        return np.where(cnt > 0, out, LD(0))

    def suffix_g(self, nskip, fast, mintime, fft=False):
        T = self.T
        origins = np.arange(0, T - 1, nskip)
        a, b = self.a - self.shift_a, self._bb() - (self.shift_b if self.b is not None else self.shift_a)
        N = (T - origins).astype(LD)
        sig2 = self._suffix_x(0, a, b)[origins] / N
        last = -1
        for n in range(T - 1):
            if self.a[n] != self.a[n + 1] or (self.b is not None and self.b[n] != self.b[n + 1]):
                last = n
        g = np.ones(origins.size, dtype=LD)
        stop = np.zeros(origins.size, np.int64)
        st = np.zeros(origins.size, np.int32)
        st[(origins > last) | (sig2 == 0)] = ZERO_VARIANCE
        tend = T - origins - (0 if fft else 1)
        run = st == 0
        end1 = run & (1 >= tend)
        st[end1], stop[end1] = END, 1
        for t, inc in _schedule(fast and not fft, T):
            run = st == 0
            if not run.any():
                break
            x = self._suffix_x(t, a, b)[origins]
            x = x + self._suffix_x(t, b, a)[origins] if self.b is not None else 2 * x
            with np.errstate(divide="ignore", invalid="ignore"):  # (zero-variance origins: not running)
                C = x / (2 * (N - t) * sig2)
            brk = run & (C <= 0) & (t > mintime)
            st[brk], stop[brk] = STOPPED, t
            upd = run & ~brk
            g[upd] += 2 * C[upd] * (1 - LD(t) / N[upd]) * inc
            fin = upd & (t + inc >= tend)
            st[fin], stop[fin] = END, t + inc
        g = np.maximum(g.astype(np.float64), 1.0)
        g[st == ZERO_VARIANCE] = 1.0
        return g, stop, st

    def _segment_sums(self, t, x, y):
        """per segment: sum over its valid pairs of x_n y_(n+t)."""
        ends = np.cumsum(self.seg)
        starts = ends - self.seg
        out = np.zeros(self.seg.size, dtype=LD)
        for k, (s0, e) in enumerate(zip(starts, ends)):
            if t < e - s0:
                out[k] = np.sum(x[s0:e - t] * y[s0 + t:e])
        return out

    def multiple_g(self, fast, mintime, want_ct=False):
        a = self.a - self.shift_a
        T = self.T
        maxN = int(self.seg.max())
        navg = LD(T) / LD(self.seg.size)
        sched = _schedule(fast, maxN)
        ct = np.zeros(len(sched) + 1) if want_ct else None
        sig2 = self._segment_sums(0, a, a).sum() / LD(T)
        if sig2 == 0:
            return 1.0, 0, ZERO_VARIANCE, ct
        g = LD(1)
        if 1 >= maxN - 1:
            return 1.0, 1, END, ct
        for k, (t, inc) in enumerate(sched, start=1):
            den = LD(np.sum(np.maximum(self.seg - t, 0)))
            C = self._segment_sums(t, a, a).sum() / den / sig2
            if want_ct:
                ct[k] = float(C)
            if C <= 0 and t > mintime:
                return max(float(g), 1.0), t, STOPPED, ct
            g += 2 * C * (1 - LD(t) / navg) * inc
            if t + inc >= maxN - 1:
                return max(float(g), 1.0), t + inc, END, ct
        raise AssertionError("schedule ended")

    def lag_sums(self, lags, origins, segments=False):
        lags = np.asarray(lags, dtype=np.int64)
        origins = np.asarray(origins, dtype=np.int64)
        xab = np.zeros((lags.size, origins.size))
        xba = np.zeros((lags.size, origins.size))
        a = self.a - self.shift_a
        b = self._bb() - (self.shift_b if self.b is not None else self.shift_a)
        for j, t in enumerate(lags):
            if segments:
                bounds = list(origins) + [self.T]
                for i in range(origins.size):
                    lo, hi = bounds[i], bounds[i + 1]
                    n = np.arange(lo, hi)
                    ok = t < self.rem[lo:hi]
                    xab[j, i] = float(np.sum(a[n[ok]] * b[n[ok] + t]))
                    xba[j, i] = float(np.sum(b[n[ok]] * a[n[ok] + t]))
            else:
                xab[j] = self._suffix_x(int(t), a, b)[origins].astype(np.float64)
                xba[j] = self._suffix_x(int(t), b, a)[origins].astype(np.float64)
        return xab, xba

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
