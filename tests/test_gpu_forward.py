"""Model.log_probability on the GPU against the extended-precision forward (tests/forward_exact.py), value by value at
forward_exact.tol: the row-blocked sum-product kernels (forward_rows.h), the column kernels with and without row tiles
(forward_columns.h) and the generic kernel (forward_generic.h), reached through the default routing, FLAG_DEEP_TILES,
FLAG_ANTIDIAGONAL and FLAG_FORCE_GENERIC.  The largest |got - exact| / tol of each route is printed at the end of the
module (run with -s to see it)."""
import math

import numpy as np
import pytest

from conftest import ALL_MODEL_GOLDENS, load_golden
from forward_exact import ExactForward, tol

pytestmark = pytest.mark.gpu

ROUTES = ["default", "deep", "antidiagonal", "generic"]
_RATIOS = {}


def _flags(route):
    from advntr_amd import _lib
    return {"default": 0, "deep": _lib.FLAG_DEEP_TILES, "antidiagonal": _lib.FLAG_ANTIDIAGONAL,
            "generic": _lib.FLAG_FORCE_GENERIC}[route]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(_RATIOS):
        print("\nforward max |got - exact| / tol  %-14s %.3g" % (k, _RATIOS[k]))


def check(got, X, reads, route, dm, label=""):
    """Every value of `got` within tol of the exact forward of its read.  Empty reads and models without a column
    program run on the generic kernel whatever the flags: they are held to its (log-domain) bound."""
    for i, s in enumerate(reads):
        want = X.logp(s)
        if math.isinf(want):
            assert math.isinf(got[i]) and got[i] < 0, (label, i, len(s), got[i])
            continue
        kind = "generic" if (route == "generic" or len(s) == 0 or not dm.has_column_program()) else "columns"
        t = tol(len(s), want, kind, depth=X.silent_depth)
        err = abs(float(got[i]) - want)
        key = route if kind != "generic" or route == "generic" else route + "/generic"
        _RATIOS[key] = max(_RATIOS.get(key, 0.0), err / t)
        assert err <= t, (label, route, i, len(s), float(got[i]), want, err, t)


def _model(loc):
    return loc.model.device_model(), ExactForward.from_arrays(loc.model.baked_arrays())


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ALL_MODEL_GOLDENS)
def test_goldens_vs_exact(name, route):
    from advntr_amd import _lib
    from test_gpu_parity import device_model_from_golden
    g = load_golden(name)
    rs = [r for r in g["reads"] if "forward_logp" in r]
    if not rs:
        pytest.skip("no forward values in this golden")
    dm, _ = device_model_from_golden(g)
    X = ExactForward.from_golden(g)
    reads = [r["seq"] for r in rs][:24]
    bases, off = _lib.encode_reads(reads)
    got = _lib.forward_batch([dm], bases, off, np.zeros(len(reads), np.int32), flags=_flags(route))
    check(got, X, reads, route, dm, name)


LENGTHS = (0, 1, 2, 4, 5, 63, 64, 65, 124, 125, 128, 129, 154, 155, 156, 192, 193, 256, 257, 320, 384, 385, 700, 1500)


@pytest.mark.parametrize("route", ROUTES)
def test_length_edges_in_a_large_mixed_batch(route):
    """Every column_launch_fwd slot, every forward_rows instantiation (a batch large enough for the row-blocked lists)
    and empty reads on the generic kernel; every value of the edge lengths, a sample of the filler."""
    from advntr_amd import _lib, workloads
    rng = np.random.default_rng(11)
    loc = workloads.make_locus(rng, 60, 17, 5, n_units=3)
    dm, X = _model(loc)
    edge = [workloads.make_reads(rng, loc, 1, n, locus_fraction=1.0)[0] if n >= 64 else workloads.rand_seq(rng, n)
            for n in LENGTHS for _ in range(2)]
    filler = workloads.make_reads(rng, loc, 600, 150) + workloads.make_reads(rng, loc, 200, 100)
    reads = filler[:300] + edge + filler[300:]
    bases, off = _lib.encode_reads(reads)
    got = _lib.forward_batch([dm], bases, off, np.zeros(len(reads), np.int32), flags=_flags(route))
    pick = list(range(300, 300 + len(edge))) + list(range(0, len(reads), 97))
    check(got[pick], X, [reads[i] for i in pick], route, dm, "lengths")


@pytest.mark.parametrize("route", ["default", "antidiagonal", "generic"])
def test_random_locus_shapes_vs_exact(route):
    """10 random loci: flank 3-150, pattern 2-40, copies 1-8 (one copy: no fan-in state), error rate 0.05 or 0.3,
    1-4 profile rows; the first is a model under 64 columns."""
    from advntr_amd import _lib, workloads
    rng = np.random.default_rng(4243)
    shapes = [(3, 2, 1)] + [(int(rng.integers(3, 151)), int(rng.integers(2, 41)), int(rng.integers(1, 9))) for _ in range(9)]
    narrow = 0
    for trial, (flank, plen, copies) in enumerate(shapes):
        loc = workloads.make_locus(rng, flank, plen, copies, float(rng.choice([0.05, 0.3])), n_units=int(rng.integers(1, 5)))
        dm, X = _model(loc)
        assert dm.has_column_program()
        narrow += dm.n_columns() < 64
        reads = [workloads.make_reads(rng, loc, 1, int(n))[0] for n in rng.integers(1, 321, 10)]
        bases, off = _lib.encode_reads(reads)
        got = _lib.forward_batch([dm], bases, off, np.zeros(len(reads), np.int32), flags=_flags(route))
        check(got, X, reads, route, dm, (trial, flank, plen, copies))
    assert narrow >= 1


def _multi_model_batch(rng):
    from advntr_amd import workloads
    loci = [workloads.make_locus(rng, f, p, c, e, n_units=u) for f, p, c, e, u in
            ((60, 17, 5, 0.05, 3), (12, 5, 2, 0.3, 1), (150, 14, 11, 0.05, 1), (30, 33, 1, 0.3, 2))]
    reads, which = [], []
    for k, loc in enumerate(loci):
        for n in (150, 150, 150, 100, 155, 60, 1, 0, 170, 300):
            reads += workloads.make_reads(rng, loc, 6, n) if n else [""]
            which += [k] * (6 if n else 1)
    perm = rng.permutation(len(reads))
    return loci, [reads[i] for i in perm], np.asarray(which, np.int32)[perm]


@pytest.mark.parametrize("route", ["default", "deep"])
def test_ragged_multi_model_batch_equals_single_model_batches(route):
    """Reads of four models in permuted order (the model changes between tiles: every change re-stages and re-exponentiates
    the LDS tables; under FLAG_DEEP_TILES reads run back to back with nothing reset between them): each value is bitwise
    what the read gets in a batch of its own model's reads on the same route, and within tol of the exact forward."""
    from advntr_amd import _lib
    rng = np.random.default_rng(77)
    loci, reads, which = _multi_model_batch(rng)
    dms = [l.model.device_model() for l in loci]
    bases, off = _lib.encode_reads(reads)
    got = _lib.forward_batch(dms, bases, off, which, flags=_flags(route))
    for k, loc in enumerate(loci):
        idx = np.nonzero(which == k)[0]
        sb, so = _lib.encode_reads([reads[i] for i in idx])
        alone = _lib.forward_batch([dms[k]], sb, so, np.zeros(len(idx), np.int32), flags=_flags(route))
        assert np.array_equal(got[idx], alone), (k, np.nonzero(got[idx] != alone)[0])
        X = ExactForward.from_arrays(loc.model.baked_arrays())
        check(got[idx], X, [reads[i] for i in idx], route, dms[k], ("model", k))


def test_resident_multi_model_batch_equals_one_shot():
    from advntr_amd import _lib
    rng = np.random.default_rng(78)
    loci, reads, which = _multi_model_batch(rng)
    dms = [l.model.device_model() for l in loci]
    bases, off = _lib.encode_reads(reads)
    one_shot = _lib.forward_batch(dms, bases, off, which)
    B = _lib.DeviceBatch(dms, bases, off, which)
    B.run()
    B.forward()
    got, _ = B.fetch()
    B.close()
    assert np.array_equal(got, one_shot)


def test_wide_models_lds_staging_levels_and_tail_weights():
    """Widths chosen from forward_lds_bytes / forward_rows_tailw_cap (column_launch.h) and batch_build's staging level
    (engine.hip).  A read-matcher column program of NC columns takes L ~ 32 NC B of LDS tables (classes and emissions are a
    few KB; the column-info and state tables 16 B per column each), core = L - 16 (NC + 2), min = core - 16 (NC + 2), and
    the batch adds pad = 16 (NC + 512) to each.  The sum-product launch adds forward_lds_bytes' 16 (NC + 128) + 32, the
    row-blocked one another 8 * 2 (NC + 64) of tail weights when that still fits 160 KiB.
      * flank 60 (NC ~ 190, L ~ 9 KB): everything staged (level 2) and the tail weights in LDS.
      * flank 2000 (NC = 4174, L = 136 880): the Viterbi sizing already leaves level 2 (L + pad = 211 856 > 160 KiB);
        the sum-product at level 1 would take core + pad + 16 (NC + 128) + 32 ~ 214 KB, at level 0 min + pad + ... ~ 147 KB:
        level 0, and 147 KB + 67 808 B of tail weights > 160 KiB: forward_rows_kernel exponentiates every tail edge per read.
      * flank 3000 (NC = 6174): min + pad + 16 (NC + 128) + 32 ~ 213 KB even at level 0: EngineError (ADVNTR_ERR_TOO_LARGE).
    A single read-matcher model does not reach forward level 1: with the 4 KB of tables the sizes above are in the ratio
    64 : 48 : 32 per column, and where level 1 would fit the Viterbi sizing has not left level 2."""
    from advntr_amd import _lib, workloads
    rng = np.random.default_rng(2000)
    for flank in (60, 2000):
        loc = workloads.make_locus(rng, flank, 25, 6, 0.05, n_units=2)
        dm, X = _model(loc)
        reads = [workloads.make_reads(rng, loc, 1, n, locus_fraction=1.0, sub_rate=0.03)[0] for n in (1, 40, 100, 150, 155, 156)]
        bases, off = _lib.encode_reads(reads)
        for route in ("default", "antidiagonal"):
            got = _lib.forward_batch([dm], bases, off, np.zeros(len(reads), np.int32), flags=_flags(route))
            check(got, X, reads, route, dm, ("flank", flank))
    loc = workloads.make_locus(rng, 3000, 25, 6, 0.05, n_units=2)
    dm = loc.model.device_model()
    assert dm.has_column_program()
    bases, off = _lib.encode_reads([workloads.rand_seq(rng, 100)])
    with pytest.raises(_lib.EngineError):
        _lib.forward_batch([dm], bases, off, np.zeros(1, np.int32))


def test_long_reads_on_the_tiled_route():
    """Reads up to 65 537 bases (341 row tiles, 341 seams in tol) on a PacBio-rate model (error rate 0.3) and on a
    0.05 one, reads of the locus with 12 % indels and substitutions and reads that match nothing."""
    from advntr_amd import _lib, workloads
    rng = np.random.default_rng(65537)
    for er in (0.3, 0.05):
        loc = workloads.make_locus(rng, 10, 8, 3, er, n_units=2)
        dm, X = _model(loc)
        unit = loc.units[0]
        reads = []
        for n in (1501, 10000, 65537):
            body = (loc.left + unit * (n // len(unit) + 1))[:n - 10] + loc.right
            reads.append(workloads.noisy_copy(rng, body, 0.12)[:n])
        reads += [workloads.rand_seq(rng, 5000), "A" * 3000]
        bases, off = _lib.encode_reads(reads)
        for route in ("default", "antidiagonal"):
            got = _lib.forward_batch([dm], bases, off, np.zeros(len(reads), np.int32), flags=_flags(route))
            check(got, X, reads, route, dm, ("long", er))


@pytest.mark.parametrize("route", ROUTES)
def test_both_strands_returns_2n_values(route):
    """FLAG_BOTH_STRANDS: 2n values, entry n + i bitwise the forward of the explicitly reverse-complemented read i."""
    from advntr_amd import _lib, vntr_finder, workloads
    rng = np.random.default_rng(32)
    loc = workloads.make_locus(rng, 40, 11, 4, n_units=2)
    dm, X = _model(loc)
    reads = workloads.make_reads(rng, loc, 70, 150) + [workloads.rand_seq(rng, n) for n in (1, 64, 200, 700)]
    bases, off = _lib.encode_reads(reads)
    which = np.zeros(len(reads), np.int32)
    got = _lib.forward_batch([dm], bases, off, which, flags=_flags(route) | _lib.FLAG_BOTH_STRANDS)
    assert got.shape == (2 * len(reads),)
    fwd = _lib.forward_batch([dm], bases, off, which, flags=_flags(route))
    rc = [vntr_finder.reverse_complement(s) for s in reads]
    rb, ro = _lib.encode_reads(rc)
    rev = _lib.forward_batch([dm], rb, ro, which, flags=_flags(route))
    assert np.array_equal(got[:len(reads)], fwd)
    assert np.array_equal(got[len(reads):], rev)
    check(got[len(reads)::9], X, rc[::9], route, dm, "reverse")
