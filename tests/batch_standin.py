"""CPU stand-in for ``pymbar_amd.batch.DeviceBatch`` -- TEST INFRASTRUCTURE ONLY.

The calls ``MBARBatch`` makes on a batch handle, on top of the numpy oracle: the solve runs every problem's state machine on the
host (``batch.step_host``, the function the device runs) with each pass evaluated by the oracle, as tests/test_mbar_batch_host.py
drives it; ``gram_w`` and the three extension-row calls are written out in numpy.  Injected where ``DeviceBatch`` is looked up
(``monkeypatch.setattr(batch, "DeviceBatch", OracleBatch)``).  Nothing under ``pymbar_amd/`` imports this.
"""
import numpy as np
from scipy.special import logsumexp

from oracle import mbar_oracle as oracle
from pymbar_amd import batch

MAX_K = batch.MAX_K


class OracleBatch:
    def __init__(self, blocks, device=None):
        self.blocks = [np.array(b, dtype=np.float64) for b in blocks]  # (an upload is a copy)
        self.device = 0 if device is None else device
        self.P = len(blocks)
        self.K = np.array([b.shape[0] for b in blocks], dtype=np.int64)
        self.N = np.array([b.shape[1] for b in blocks], dtype=np.int64)
        self.R = np.zeros(self.P, dtype=np.int64)
        self.rows = [None] * self.P
        self.Nk = [None] * self.P
        self.closed = False
        self.calls = dict(solve=0, gram_w=0, set_ext=0, ext_lognum=0, ext_gram=0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.closed = True

    def _logden(self, p, f):
        return oracle.log_denominator(self.blocks[p], self.Nk[p], f)

    def solve(self, states):
        self.calls["solve"] += 1
        passes = 0
        for p in range(self.P):
            st, K, u = states[p], int(self.K[p]), self.blocks[p]
            N_k = np.array(st.Nk[:K], dtype=np.float64)
            self.Nk[p] = N_k
            st.phase, st.status = 0, batch.RUNNING
            batch.step_host(st)
            while st.status == batch.RUNNING:
                reqs = [np.array(st.req[r][:K]) for r in range(st.nreq)]
                ln = np.stack([logsumexp(-oracle.log_denominator(u, N_k, f) - u, axis=1) for f in reqs])
                G = None
                if st.gram_req >= 0:
                    pm = N_k * oracle.mbar_W_nk(u, N_k, reqs[st.gram_req])
                    G = pm.T @ pm
                batch.step_host(st, ln, G)
                passes += 1
        return passes

    def _W(self, p, f):
        return np.exp(f[:, None] - self.blocks[p] - self._logden(p, f)[None, :]).T

    def gram_w(self, F, mask):
        self.calls["gram_w"] += 1
        gram, wsum = [], []
        for p in range(self.P):
            K = int(self.K[p])
            if mask[p]:
                W = self._W(p, np.asarray(F[p][:K], dtype=np.float64))
                gram.append((W.T @ W).ravel())
                wsum.append(W.sum(0))
            else:
                gram.append(np.zeros(K * K))
                wsum.append(np.zeros(K))
        return np.concatenate(gram), np.concatenate(wsum)

    def set_ext(self, rows):
        self.calls["set_ext"] += 1
        if rows is None:
            rows = [None] * self.P
        self.rows = [None if r is None or len(r) == 0 else np.array(r, dtype=np.float64) for r in rows]
        self.R = np.array([0 if r is None else r.shape[0] for r in self.rows], dtype=np.int64)
        for p, r in enumerate(self.rows):
            assert r is None or (r.shape[1] == self.N[p] and self.K[p] + r.shape[0] <= batch.MAX_AUG)
            assert r is None or not (np.any(np.isnan(r)) or np.any(r == -np.inf))

    def ext_lognum(self, F, mask):
        self.calls["ext_lognum"] += 1
        out = []
        for p in range(self.P):
            if mask[p] and self.R[p] > 0:
                ld = self._logden(p, np.asarray(F[p][:int(self.K[p])], dtype=np.float64))
                out.append(logsumexp(-ld[None, :] - self.rows[p], axis=1))
            else:
                out.append(np.zeros(int(self.R[p])))
        return np.concatenate(out)

    def ext_gram(self, F, f_ext, mask, group_bytes=0):
        self.calls["ext_gram"] += 1
        roff = np.concatenate(([0], np.cumsum(self.R)))
        gram, wsum = [], []
        for p in range(self.P):
            K, A = int(self.K[p]), int(self.K[p] + self.R[p])
            if mask[p]:
                f = np.asarray(F[p][:K], dtype=np.float64)
                Q = self._W(p, f)
                if self.R[p] > 0:
                    fe = np.asarray(f_ext[roff[p]:roff[p + 1]], dtype=np.float64)
                    assert np.all(np.isfinite(fe))
                    Q = np.hstack([Q, np.exp(fe[:, None] - self.rows[p] - self._logden(p, f)[None, :]).T])
                gram.append((Q.T @ Q).ravel())
                wsum.append(Q.sum(0))
            else:
                gram.append(np.zeros(A * A))
                wsum.append(np.zeros(A))
        return np.concatenate(gram), np.concatenate(wsum)
