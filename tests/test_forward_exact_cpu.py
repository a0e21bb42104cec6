"""The extended-precision forward reference (tests/forward_exact.py) and the tolerance the sum-product kernels are held
to (forward_exact.tol), checked without a GPU: against the reference's own log_probability values (goldens), against
mpmath at 40 digits, against the fp64 oracle within the oracle's bound, and against the column program's scalar
sum-product (oracle/colprog_check.cpp) at the tight bound.  The sensitivity test shows that the bound catches a model
with one in-edge missing or one transition class off by 1e-9 relative, which the old 1e-9 relative bar did not."""
import math

import numpy as np
import pytest

from conftest import ALL_MODEL_GOLDENS, load_golden
from forward_exact import ExactForward, tol


def _arrays_without_edge(a, k):
    """Baked arrays of the same model with CSR in-edge k removed."""
    b = dict(a)
    b["in_src"] = np.delete(a["in_src"], k)
    b["in_logp"] = np.delete(a["in_logp"], k)
    dst = np.searchsorted(a["in_ptr"], k, side="right") - 1
    ptr = np.array(a["in_ptr"], np.int64)
    ptr[dst + 1:] -= 1
    b["in_ptr"] = ptr
    return b


def _oracle(a):
    from oracle.oracle import OracleModel
    edges = [(int(a["in_src"][k]), l, float(a["in_logp"][k])) for l in range(a["m"])
             for k in range(a["in_ptr"][l], a["in_ptr"][l + 1])]
    return OracleModel(a["m"], a["silent_start"], a["start_index"], a["end_index"], edges, a["emis_logp"])


def mp_forward(a, seq, dps=40):
    """oracle_forward's recurrence in mpmath (log domain, 40 significant digits): tiny models only."""
    import mpmath
    from oracle.oracle import encode
    x = encode(seq)
    with mpmath.workdps(dps):
        m, p, st, en = a["m"], a["silent_start"], a["start_index"], a["end_index"]
        ptr, src = a["in_ptr"], a["in_src"]
        w = [mpmath.exp(mpmath.mpf(float(v))) for v in a["in_logp"]]
        em = np.asarray(a["emis_logp"], np.float64).reshape(p, 4)
        f = [mpmath.mpf(0)] * m
        f[st] = mpmath.mpf(1)
        for l in range(p, m):
            if l != st:
                f[l] = mpmath.fsum(f[src[k]] * w[k] for k in range(ptr[l], ptr[l + 1]) if p <= src[k] < l)
        for c in x:
            g = [mpmath.mpf(0)] * m
            for l in range(p):
                g[l] = mpmath.fsum(f[src[k]] * w[k] for k in range(ptr[l], ptr[l + 1])) * mpmath.exp(mpmath.mpf(float(em[l, c])))
            for l in range(p, m):
                g[l] = mpmath.fsum(g[src[k]] * w[k] for k in range(ptr[l], ptr[l + 1]) if src[k] < p or src[k] < l)
            f = g
        v = f[en] if ptr[en + 1] != ptr[en] else mpmath.fsum(f[:p])
        return float(mpmath.log(v)) if v > 0 else -math.inf


def test_tolerance_targets():
    """The bound is <= 1e-11 nats for a 150-base read at logp ~ -300, and at least 1 000x tighter than the old
    1e-9 |logp| at every length."""
    assert tol(150, -300.0, "rows") <= 1e-11 and tol(150, -300.0, "columns") <= 1e-11
    for n in (1, 150, 192, 193, 1500, 10000, 65537, 100000):
        logp = -2.0 * n                      # the typical rate; a rate of ~-1.4 nats per base (match everything) is larger
        for route in ("rows", "columns"):
            assert tol(n, logp, route) <= 1e-3 * 1e-9 * max(1.0, abs(logp)), (n, route)


@pytest.mark.parametrize("name", ALL_MODEL_GOLDENS)
def test_exact_forward_matches_reference_goldens(name):
    """The reference's own log_probability (pomegranate, fp64 log domain) at 1e-14 relative."""
    g = load_golden(name)
    rs = [r for r in g["reads"] if "forward_logp" in r]
    if not rs:
        pytest.skip("no forward values in this golden")
    X = ExactForward.from_golden(g)
    for r in rs[:24]:
        want, got = r["forward_logp"], X.logp(r["seq"])
        if math.isinf(want):
            assert math.isinf(got) and got < 0
        else:
            assert abs(got - want) <= 1e-14 * max(1.0, abs(want)), (name, len(r["seq"]), got, want)


def test_dense_and_sparse_modes_agree():
    g = load_golden("p6_f100_c17")
    D, S = ExactForward.from_golden(g, dense=True), ExactForward.from_golden(g, dense=False)
    for r in g["reads"][:4]:
        a, b = D.logp_ld(r["seq"]), S.logp_ld(r["seq"])
        assert abs(float(a - b)) <= 1e-16 * abs(float(a)), (a, b)


def test_exact_forward_vs_mpmath():
    """The toy golden, the two generic goldens and small random loci (single copy, multi-row profiles, both error rates)
    against a 40-digit restatement: agreement to a few long-double ulps, far below the fp64 bound."""
    from advntr_amd import workloads
    from oracle.oracle import OracleModel
    cases = []
    for name in ("toy_f8_l5_c2", "generic_finite", "generic_infinite"):
        g = load_golden(name)
        O = OracleModel.from_golden(g)
        in_ptr, in_src, in_logp, _ = O.csr()
        gm = g["model"]
        a = dict(m=O.m, silent_start=gm["silent_start"], start_index=gm["start_index"], end_index=gm["end_index"],
                 in_ptr=in_ptr, in_src=in_src, in_logp=in_logp, emis_logp=O.emis)
        cases.append((a, [r["seq"] for r in g["reads"][:3]] + [""]))
    rng = np.random.default_rng(40)
    for flank, plen, copies, er, rows in ((3, 2, 1, 0.3, 1), (5, 4, 2, 0.05, 3), (4, 3, 3, 0.3, 2)):
        loc = workloads.make_locus(rng, flank, plen, copies, er, n_units=rows)
        cases.append((loc.model.baked_arrays(), [workloads.rand_seq(rng, n) for n in (1, 7, 20)] + [""]))
    for a, reads in cases:
        X = ExactForward.from_arrays(a)
        for s in reads:
            want, got = mp_forward(a, s), X.logp(s)
            if math.isinf(want):
                assert math.isinf(got) and got < 0
            else:
                assert abs(got - want) <= 1e-16 * max(1.0, abs(want)), (len(s), got, want)


def test_oracle_within_its_log_domain_bound():
    """The fp64 oracle (pair_lse folding, the generic kernel's arithmetic) stays within tol(..., "generic") of the exact
    value, short and long reads: the bound the generic route is held to covers the reference arithmetic itself."""
    from advntr_amd import workloads
    rng = np.random.default_rng(9)
    loc = workloads.make_locus(rng, 40, 12, 4, 0.3, n_units=2)
    a = loc.model.baked_arrays()
    O, X = _oracle(a), ExactForward.from_arrays(a)
    unit = loc.units[0]
    reads = workloads.make_reads(rng, loc, 6, 150) + [workloads.rand_seq(rng, 700)]
    reads.append(workloads.noisy_copy(rng, loc.left + unit * 150 + loc.right, 0.12)[:2500])
    worst = 0.0
    for s in reads:
        want = X.logp(s)
        err = abs(O.forward(s) - want)
        worst = max(worst, err / tol(len(s), want, "generic", depth=X.silent_depth))
    assert worst <= 1.0, worst


def test_column_program_forward_at_the_tight_bound():
    """colprog_forward (the column program evaluated in the forward kernels' fold order, log domain) on random locus
    shapes against the exact forward: a column-program compiler error in the sum-product (a lost edge, a wrong class)
    shows up here without a GPU."""
    from advntr_amd import workloads
    from oracle.oracle import encode
    from test_colprog_cpu import checker
    L = checker()
    rng = np.random.default_rng(31)
    for trial in range(8):
        flank, plen, copies = int(rng.integers(3, 60)), int(rng.integers(2, 30)), int(rng.integers(1, 8))
        loc = workloads.make_locus(rng, flank, plen, copies, float(rng.choice([0.05, 0.3])), n_units=int(rng.integers(1, 5)))
        a = loc.model.baked_arrays()
        h = L.colprog_create(a["m"], a["silent_start"], a["start_index"], a["end_index"], len(a["in_src"]),
                             a["in_ptr"].ctypes.data, a["in_src"].ctypes.data, a["in_logp"].ctypes.data,
                             a["emis_logp"].ctypes.data)
        assert L.colprog_valid(h), L.colprog_why(h)
        X = ExactForward.from_arrays(a)
        reads = workloads.make_reads(rng, loc, 4, int(rng.integers(1, 200))) + [workloads.rand_seq(rng, 150)]
        for s in reads:
            codes = encode(s)
            got = L.colprog_forward(h, codes.ctypes.data, len(codes))
            want = X.logp(s)
            assert abs(got - want) <= tol(len(s), want, "generic", depth=X.silent_depth), (trial, flank, plen, copies, len(s), got, want)
        L.colprog_destroy(h)


def test_tolerance_catches_single_edge_and_class_errors():
    """Sensitivity: on the 60/17/5 locus of the GPU forward sweep, delete one random in-edge (60 trials) or scale the
    transitions of one class of edges by 1 + 1e-9 (the classes named by their source / destination kinds), and
    compare exact forwards on six 150-base reads.  The tight bound must see the change in nearly every trial, including
    trials the old 1e-9 relative bound could not see."""
    from advntr_amd import workloads
    rng = np.random.default_rng(8)
    loc = workloads.make_locus(rng, 60, 17, 5, n_units=3)
    reads = workloads.make_reads(rng, loc, 6, 150, locus_fraction=1.0)
    a = loc.model.baked_arrays()
    X = ExactForward.from_arrays(a)
    base = [X.logp(s) for s in reads]
    n_edges = int(a["in_ptr"][-1])
    caught = missed_by_old = caught_and_missed_by_old = 0
    trials = 60
    for k in rng.choice(n_edges, trials, replace=False):
        Y = ExactForward.from_arrays(_arrays_without_edge(a, int(k)))
        shift = [abs(Y.logp(s) - b) for s, b in zip(reads, base)]
        hit = any(d > tol(150, b, "rows") for d, b in zip(shift, base))
        old = all(d <= 1e-9 * max(1.0, abs(b)) for d, b in zip(shift, base))
        caught += hit
        missed_by_old += old
        caught_and_missed_by_old += hit and old
    # (measured: 56 / 60 caught, the other 4 edges lie on no path of these reads and move nothing; the old bar missed 13
    # of the 60, 9 of which the new bound catches)
    assert caught >= 0.9 * trials, caught
    assert missed_by_old >= 3 and caught_and_missed_by_old >= 2, (missed_by_old, caught_and_missed_by_old)
    # one transition class off by 1e-9 relative: emitting -> emitting, emitting -> silent, silent -> anything
    dst = np.repeat(np.arange(a["m"]), np.diff(a["in_ptr"]))
    p = a["silent_start"]
    for sel in ((dst < p) & (a["in_src"] < p), (dst >= p) & (a["in_src"] < p), a["in_src"] >= p):
        b = dict(a)
        b["in_logp"] = np.where(sel, a["in_logp"] + math.log1p(1e-9), a["in_logp"])
        Y = ExactForward.from_arrays(b)
        shift = [abs(Y.logp(s) - v) for s, v in zip(reads, base)]
        assert max(shift) > 100 * tol(150, max(base, key=abs), "rows"), shift
