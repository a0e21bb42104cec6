"""Extended-precision forward: Model.log_probability (hmm.pyx:1371-1484, 1300-1313) in np.longdouble, linear domain.

TEST INFRASTRUCTURE, the reference the sum-product kernels are measured against.  The recurrence is oracle_forward's
(oracle/viterbi_oracle.c), restated without the log domain:
  - row 0: the start state holds 1; the other silent states, in index order, collect from silent states of lower index;
  - row i (1..n): an emitting state l collects every in-edge from row i-1 and is multiplied by its emission of x_i; then
    the silent states, in index order, collect from the emitting states of row i and from silent states of lower index;
  - a finite model (its end state has in-edges) ends at the end state of row n, an infinite one at the sum of the
    emitting states of row n; an empty read gives row 0's value.
Every row is rescaled by its largest value and the scale kept as a long-double logarithm, so no read underflows.

Dense mode folds the silent closure into a row-transfer matrix: s = W e (W by forward substitution over the strictly lower
triangular silent->silent edges), M = T_ee + T_es W, and each row is e <- emis[:, x] * (M @ e).  Sparse mode (models too
wide for dense matrices) takes the silent states level by level in the topological order of the silent->silent edges.
"""
import numpy as np

LD = np.longdouble
if np.finfo(LD).eps > 1e-18:
    raise ImportError("forward_exact needs an extended-precision long double (eps %g)" % np.finfo(LD).eps)

U = 2.0 ** -53                   # unit roundoff of fp64

DENSE_MAX_EMITTING = 256         # dense p x p products cost p^2 per row; past this the level-by-level sparse mode is faster


def tol(n, logp, route, seams=None, depth=1):
    """Bound on |kernel - exact| (nats) for a read of n bases whose exact log-probability is logp.

    Error model (u = 2^-53).  Linear-domain routes ("rows": forward_rows.h; "columns": forward_columns.h):
      * each row is a sum of positive terms times positive weights, so every cell carries a relative error of a few u
        per row (one fma chain per in-edge class, the emission product, the exp of each table entry made once at staging,
        which is a fixed relative error per factor, not per row); these compound additively in relative terms, i.e.
        additively in the log: 64 u per row covers up to ~64 roundings per row on the path, far above the ~10-20 of a
        read-matcher cell (+ 64 u n);
      * the tail states fold the last row in fp64 and take one log (the rows route) or log-domain pair_lse (columns): a
        few u relative, i.e. a few u absolute in logp (inside the 1e-13 floor);
      * every row-tile seam of the tiled column route takes the row to the log domain and back (col_row_to_log): a
        value near logp is rounded in the log domain, an absolute error of u |logp| per value, amplified by the exp
        (16 u |logp| per seam covers the few values a cell sums after the seam);
      * 16 u |logp| more for the final scale (rows x log 16) subtracted from log(result), and a 1e-13 floor for libm's
        1-ulp log / exp on values of order 1..1000.
    Log-domain route ("generic": forward_generic.h, and the fp64 oracle): every pair_lse / addition of a transition
    rounds the running log value, an absolute error of u |value| per fold, and the running value's magnitude grows to
    |logp| along the path: 2 u |logp| per fold on the path, plus the same floor.  A path folds once per row and once per
    silent state it passes in a chain of silent states: depth = the longest silent -> silent chain of the model
    (ExactForward.silent_depth; the deletion chain across the model in a read matcher).  Counting only the n rows
    underestimated the empty read, whose value is row 0's fold down that chain (measured on the GPU: 16 u |logp| on a
    ~200-column model, 4x the n = 1 allowance): the bound is 2 u |logp| (n + depth).
    """
    a = abs(float(logp)) if np.isfinite(logp) else 0.0
    if route == "generic":
        return 1e-13 + 2.0 * U * a * (n + depth)
    if seams is None:
        seams = max(0, -(-n // 192) - 1) if route == "columns" else 0
    return 1e-13 + 64.0 * U * n + 16.0 * U * a * (1 + seams)


class ExactForward(object):
    """Exact (long double) forward of a baked model given as CSR in-edge arrays (model.baked_arrays(), or the
    OracleModel.csr() of a golden)."""

    def __init__(self, m, silent_start, start_index, end_index, in_ptr, in_src, in_logp, emis_logp, dense=None):
        self.m, self.p = int(m), int(silent_start)
        self.start, self.end = int(start_index), int(end_index)
        in_ptr = np.asarray(in_ptr, np.int64)
        in_src = np.asarray(in_src, np.int64)[:in_ptr[-1]]
        w = np.exp(np.asarray(in_logp, np.float64)[:in_ptr[-1]].astype(LD))
        dst = np.repeat(np.arange(self.m), np.diff(in_ptr))
        self.finite = in_ptr[self.end + 1] != in_ptr[self.end]
        p = self.p
        self.emis = np.exp(np.asarray(emis_logp, np.float64).reshape(p, 4).astype(LD)).T.copy()    # [symbol, state]
        self.dense = (p <= DENSE_MAX_EMITTING) if dense is None else dense
        ns = self.m - p
        # the four edge classes; a silent->silent edge counts only from a lower index (the reference's single pass)
        ee = (dst < p) & (in_src < p)
        es = (dst < p) & (in_src >= p)
        se = (dst >= p) & (in_src < p)
        ss = (dst >= p) & (in_src >= p) & (in_src < dst)
        # row 0: silent values, start = 1, the others from lower-index silent states (the start state is not recomputed)
        s0 = np.zeros(ns, LD)
        s0[self.start - p] = 1 if self.start >= p else 0
        ss_ptr = [np.nonzero(ss & (dst == p + j))[0] for j in range(ns)]
        for j in range(ns):
            if p + j == self.start:
                continue
            k = ss_ptr[j]
            if len(k):
                s0[j] = np.sum(s0[in_src[k] - p] * w[k])
        if self.start < p:       # an emitting start state (not a reference shape): row 0 then holds it alone
            raise ValueError("forward_exact: the start state must be silent")
        self.s0 = s0
        level = np.zeros(ns, np.int64)              # longest chain of (counted) silent -> silent edges into each silent state
        for j in range(ns):
            k = ss_ptr[j]
            if len(k):
                level[j] = 1 + level[in_src[k] - p].max()
        self.silent_depth = int(level.max()) + 1 if ns else 0
        if self.dense:
            Tee = np.zeros((p, p), LD)
            np.add.at(Tee, (dst[ee], in_src[ee]), w[ee])
            self.Tes = np.zeros((p, ns), LD)
            np.add.at(self.Tes, (dst[es], in_src[es] - p), w[es])
            Ase = np.zeros((ns, p), LD)
            np.add.at(Ase, (dst[se] - p, in_src[se]), w[se])
            W = np.zeros((ns, p), LD)
            for j in range(ns):                        # forward substitution: W[j] = Ase[j] + sum_{k<j} Ass[j, k] W[k]
                row = Ase[j].copy()
                for k in ss_ptr[j]:
                    row += w[k] * W[in_src[k] - p]
                W[j] = row
            self.W = W
            self.M = Tee + self.Tes @ W
        else:
            # sparse: emitting states gather every in-edge of the previous row; silent states by topological level
            order = np.argsort(dst, kind="stable")
            self.e_src, self.e_w = in_src[order][(dst[order] < p)], w[order][(dst[order] < p)]
            cnt = np.bincount(dst[dst < p], minlength=p)
            self.e_has = cnt > 0
            self.e_seg = (np.cumsum(cnt) - cnt)[self.e_has]          # segment starts of the states that have in-edges
            self.levels = []
            keep = se | ss
            for lv in range(int(level.max()) + 1 if ns else 0):
                states = np.nonzero(level == lv)[0] + p
                k = np.nonzero(keep & np.isin(dst, states))[0]
                k = k[np.argsort(dst[k], kind="stable")]
                if not len(k):
                    continue
                d = dst[k]
                first = np.concatenate([[0], np.nonzero(np.diff(d))[0] + 1])
                self.levels.append((d[first], in_src[k], w[k], first))

    @classmethod
    def from_arrays(cls, a, **kw):
        return cls(a["m"], a["silent_start"], a["start_index"], a["end_index"], a["in_ptr"], a["in_src"], a["in_logp"],
                   a["emis_logp"], **kw)

    @classmethod
    def from_golden(cls, g, **kw):
        from oracle.oracle import OracleModel
        O = OracleModel.from_golden(g)
        in_ptr, in_src, in_logp, _ = O.csr()
        gm = g["model"]
        return cls(O.m, gm["silent_start"], gm["start_index"], gm["end_index"], in_ptr, in_src, in_logp, O.emis, **kw)

    def _silent(self, e):
        """Silent values of a row whose emitting values are e (sparse mode)."""
        v = np.zeros(self.m, LD)
        v[:self.p] = e
        for d, src, w, first in self.levels:
            v[d] = np.add.reduceat(v[src] * w, first)
        return v

    def logp(self, seq):
        """Exact log-probability (a Python float rounded from long double) of a read: str of ACGT or codes 0..3.
        Values of str reads are remembered (tests check one read on several routes)."""
        if not isinstance(seq, str):
            return float(self.logp_ld(seq))
        cache = self.__dict__.setdefault("_cache", {})
        if seq not in cache:
            cache[seq] = float(self.logp_ld(seq))
        return cache[seq]

    def logp_ld(self, seq):
        if isinstance(seq, str):
            from oracle.oracle import encode
            seq = encode(seq)
        x = np.asarray(seq, np.int64)
        n, p = len(x), self.p
        if n == 0:
            if self.finite:
                v = self.s0[self.end - p] if self.end >= p else LD(0)
                return np.log(v) if v > 0 else LD(-np.inf)
            return LD(-np.inf)
        scale = LD(0)
        if self.dense:
            e = self.emis[x[0]] * (self.Tes @ self.s0)
            for i in range(1, n + 1):
                c = e.max()
                if not c > 0:
                    return LD(-np.inf)
                e = e / c
                scale += np.log(c)
                if i == n:
                    break
                e = self.emis[x[i]] * (self.M @ e)
            if self.finite:
                f = self.W[self.end - p] @ e if self.end >= p else e[self.end]
            else:
                f = e.sum()
        else:
            v = np.zeros(self.m, LD)
            v[p:] = self.s0
            for i in range(n):
                g = np.zeros(p, LD)
                g[self.e_has] = np.add.reduceat(v[self.e_src] * self.e_w, self.e_seg)
                e = self.emis[x[i]] * g
                c = e.max()
                if not c > 0:
                    return LD(-np.inf)
                e = e / c
                scale += np.log(c)
                v = self._silent(e)
            f = v[self.end] if self.finite else v[:p].sum()
        return np.log(f) + scale if f > 0 else LD(-np.inf)
