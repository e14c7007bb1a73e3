"""`egp_gemm_f32` (csrc/egp_gemm.hip) against an independent float64 statement of every product, at the shapes where
the persistent kernel's item stream, its gathers / scatters, split-K with a riding remainder and the thin kernels take
paths that tests/test_gemm_gpu.py does not reach.

Reference: operands rounded to float32, then `A64 @ B64` in float64 on the GPU (gathers formed with index_select / cat,
scatters with `ref[idx] = ...` on a float64 copy of the prefilled destination); nothing of it goes through
egopose_amd.gemm. Yardstick: torch's float32 product of the same operands. Two figures per comparison:
  rel  = |got - ref| / |ref| (Frobenius)                 against  max(C x rel of the yardstick, FLOOR)
  elem = max |got - ref| / (|A| @ |B| [+ |bias|, |out|])  against  a constant E
Three-piece products without split-K keep the bounds the project already holds them to (C_DIRECT = 3, FLOOR = 2e-7,
E_DIRECT = 8e-7). For split-K products and for the thin float32 kernels the factors are measured, not assumed: the worst
HIP / yardstick ratio (over the comparisons whose HIP error is above FLOOR; below it the floor decides) and the worst
elem over every case of this file on the MI355X, doubled and rounded up. Every test prints its figures (pytest -s).

Measured on the MI355X, persistent and classic kernel together (worst HIP / yardstick ratio of rel among the comparisons
above FLOOR; worst elem):
  group 1  item stream, 128-column tiles      ratio 0.88   elem 4.2e-7
  group 2  item stream with empty slots       ratio 0.88   elem 3.5e-7
  group 3  64-column tiles                    ratio 0.85   elem 3.6e-7
  group 7  operands scaled by 2^+-20          ratio 0.88   elem 3.5e-7
  group 5  gathers / scatters, no split-K     ratio 1.46   elem 2.9e-7
  group 4  split-K with a riding remainder    ratio 0.88   elem 1.2e-7
  group 5k gathers along k, split-K           ratio 2.91   elem 3.0e-7   (the bias column of 1005 k rows summed in one range)
    -> C_SPLIT = 6 (2 x 2.91, rounded up), E_SPLIT = 6e-7 (2 x 3.0e-7)
  group 6  thin kernels, >= 64 outputs        ratio 1.10   elem 1.4e-7   (k_colsum, K = 9001 in one range)
    -> C_THIN = 3 (2 x 1.10, rounded up), E_THIN = 3e-7 (2 x 1.4e-7, rounded up)
A thin-kernel output of fewer than THIN_MIN_NUMEL = 64 elements is held to the elementwise bound alone: the ratio of two
round-off errors over one or three numbers is not a statistic (measured: 239 for the one-element bias sum of 9001 terms,
HIP 2.2e-7 against a yardstick that happened to land within 9e-10; 15 for a 1 x 1 product of K = 31; up to 5 for M = 3).

Self-checks (test_tolerance_tells_a_wrong_answer, float64 on the CPU, no kernel): a wrong answer must miss the tolerance
by at least SELF_MARGIN = 3 in rel or in elem: (a) A truncated to 16 mantissa bits (a lost third piece), (b) the k
columns [kend - 32, kbeg + 32 (nst - 1)) of one 128-row tile added a second time (a tail tile whose head was not
zeroed), (c) a 128 x 128 output tile taken from the neighbouring item, (d) one gather / scatter index shifted by one row.
Measured margins: (a) 19 (direct), 18 (gather), 6 (split-K), 34 (thin); (b) 1.5e5 and more; (c) 6e5 and more; (d) 9e5 and more.

Kernels the profiler saw: groups 1, 2, 3 k_gemm_ws alone (k_gemm_bf16x alone with EGP_GEMM_WS=0); group 4 the same +
k_gemm_reduce; group 5 k_gemm_ws (+ k_gemm_reduce with split-K), refused with EGP_GEMM_WS=0; group 6 k_gemv_rows, k_rank1,
k_colsum + k_gemm_reduce; the two neighbours k_gemm_ws / k_gemm_bf16x (M = 1) and k_gemm_bf16x (N = 1), no thin kernel.

Which kernel ran is confirmed with torch.profiler (test_profiler_sees_the_expected_kernels), and every "items per
workgroup" / "remainder rides" precondition is recomputed in the test from gemm.usable_cus() and the launcher's
arithmetic (`_Plan`), so that a change of pick_splits or of the tile sizes fails a test instead of testing less.
"""
import math

import pytest
import torch

gpu = pytest.mark.gpu

C_DIRECT, E_DIRECT = 3.0, 8e-7      # three-piece products without split-K (as tests/test_gemm_gpu.py)
C_SPLIT, E_SPLIT = 6.0, 6e-7        # split-K products and their bias-gradient column (measured, see above)
C_THIN, E_THIN = 3.0, 3e-7          # k_gemv_rows / k_rank1 / k_colsum (measured, see above)
FLOOR = 2e-7
THIN_MIN_NUMEL = 64                 # thin-kernel outputs smaller than this are held to the elementwise bound alone (see above)
SELF_MARGIN = 3.0
KERNELS = ("k_gemm_ws", "k_gemm_bf16x", "k_gemv_rows", "k_rank1", "k_colsum", "k_gemm_reduce")
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
SENTINEL = -777.25
BM, BK = 128, 32


@pytest.fixture(params=["ws", "classic"], autouse=True)
def three_piece_kernel(request, monkeypatch):
    """terms = 6 on the persistent kernel (k_gemm_ws) or, with EGP_GEMM_WS=0, on k_gemm_bf16x: every test runs both ways.
    The classic kernel must give float32-class results too, and must refuse gather / scatter operands."""
    monkeypatch.setenv("EGP_GEMM_WS", "1" if request.param == "ws" else "0")
    return request.param


# ------------------------------------------------------------------------------------------- the launcher's arithmetic

class _Plan:
    """egp_gemm_f32's tiling of an (M, N, K) product with `splits` and the ones column (egp_gemm.hip, the launcher)."""

    def __init__(self, M, N, K, splits=1, ones=False):
        n_out = N + (1 if ones else 0)
        self.bn = 64 if n_out <= 64 else 128
        self.tiles_m, self.tiles_n = -(-M // BM), -(-n_out // self.bn)
        self.tiles = self.tiles_m * self.tiles_n
        self.xcd_order = self.tiles_m >= 64
        self.slots = (-(-self.tiles_m // 8) * 8 if self.xcd_order else self.tiles_m) * self.tiles_n
        kt = -(-K // BK)
        self.k_per_split = max(1, -(-kt // max(splits, 1))) * BK
        self.ranges = -(-K // self.k_per_split)
        self.rem = K - (self.ranges - 1) * self.k_per_split                    # length of the last range
        self.rides = self.ranges > 1 and self.rem < BK
        self.written = self.ranges - 1 if self.rides else self.ranges          # splits written by k_gemm_ws
        self.items = self.tiles * self.written
        self.ktiles = -(-min(K, self.k_per_split) // BK)                       # k-tiles of a full range

    def per_workgroup(self):
        from egopose_amd.gemm import usable_cus
        return self.items / usable_cus()


# ------------------------------------------------------------------------------------------------------- comparisons

_WORST = {}


def _rel(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


def _figures(got, ref, yard, mag):
    d = (got.double() - ref).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf"), _rel(yard, ref), float("inf")
    return _rel(got, ref), _rel(yard, ref), float((d / mag.clamp_min(1e-300)).max())


def _tolerance(kind):
    return {"direct": (C_DIRECT, E_DIRECT), "split": (C_SPLIT, E_SPLIT), "thin": (C_THIN, E_THIN)}[kind]


def _check(group, what, got, ref, yard, mag, kind="direct"):
    """One comparison: prints its figures, records the group's worst ones, asserts the tolerance of `kind`."""
    c, e_max = _tolerance(kind)
    e, y, el = _figures(got, ref, yard, mag)
    few = kind == "thin" and ref.numel() < THIN_MIN_NUMEL
    w = _WORST.setdefault(group, [0.0, 0.0])
    if e > FLOOR and not few:
        w[0] = max(w[0], e / max(y, 1e-300))
    w[1] = max(w[1], el)
    print("  [%s] %-58s hip %.2e  f32 %.2e  ratio %5.2f  elem %.2e%s" % (group, what, e, y, e / max(y, 1e-300), el, "  (elem only)" if few else ""))
    assert (few or e < max(c * y, FLOOR)) and el <= e_max, (group, what, e, y, el)


def _margin(wrong, ref, yard, mag, kind):
    """How many times a known-wrong float64 result misses the tolerance (in rel or in elem, whichever misses more)."""
    c, e_max = _tolerance(kind)
    e, y, el = _figures(wrong, ref, yard, mag)
    return max(e / max(c * y, FLOOR), el / e_max)


def _report(group):
    w = _WORST.get(group, [0.0, 0.0])
    print("  [%s] worst so far: ratio %.2f  elem %.2e" % (group, w[0], w[1]))


# ---------------------------------------------------------------------------------------------------------- operands

def _gen(seed, device="cuda"):
    return torch.Generator(device=device).manual_seed(seed)


def _operands(M, N, K, a_kc, b_kc, seed, device="cuda", scale=None):
    """float32 A and B in the asked layouts and their float64 images A64 (M, K), B64 (K, N)."""
    g = _gen(seed, device)
    A = torch.randn(M, K, device=device, generator=g)
    B = torch.randn(K, N, device=device, generator=g)
    if scale is not None:                                  # exact: powers of two
        A, B = A * scale, B / scale.unsqueeze(1)
    A64, B64 = A.double(), B.double()
    return (A if a_kc else A.t().contiguous()), (B.t().contiguous() if b_kc else B), A64, B64


def _epilogue(z, bias=None, relu=False, mask=None):
    if bias is not None:
        z = z + bias.to(z.dtype)
    if relu:
        z = z.clamp_min(0)
    if mask is not None:
        z = z * (mask > 0)
    return z


def _product(A64, B64, bias=None, relu=False, mask=None):
    """(float64 reference, float32 yardstick, magnitude |A| @ |B| + |bias|) of one product with its epilogue."""
    ref = _epilogue(A64 @ B64, bias, relu, mask)
    yard = _epilogue(A64.float() @ B64.float(), bias, relu, mask)
    mag = A64.abs() @ B64.abs()
    if bias is not None:
        mag = mag + bias.double().abs()
    return ref, yard, mag


def _kernels_of(fn):
    """Names of KERNELS that the profiler records while fn() runs."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    keys = [e.key for e in prof.key_averages()]
    return {k for k in KERNELS if any(k in key for key in keys)}


def _tiled(kind):
    """The tiled kernel the fixture selects, and the one it excludes."""
    return ("k_gemm_ws", "k_gemm_bf16x") if kind == "ws" else ("k_gemm_bf16x", "k_gemm_ws")


# ------------------------------------------------------------------------------------- groups 1, 7: the item stream

@gpu
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("K,epilogue", [(32, False), (32, True), (40, False), (64, False), (95, False), (161, False), (222, False)])
def test_item_stream_128_column_tiles(a_kc, b_kc, K, epilogue):
    """M = 8000 x N = 1664: 63 x 13 = 819 items (no xcd_order), at least 3 per persistent workgroup, with 1, 2, 2, 3, 6 and 7
    k-tiles per item: the ring of 4 register sets / 2 LDS buffers is in a different phase at every item boundary, and every
    tail length occurs. K = 32 with bias + ReLU + mask: every iteration ends in an epilogue."""
    from egopose_amd.gemm import gemm
    M, N = 8000, 1664
    p = _Plan(M, N, K)
    assert not p.xcd_order and p.slots == p.tiles == 819 and p.per_workgroup() >= 3 and p.written == 1
    assert p.ktiles == {32: 1, 40: 2, 64: 2, 95: 3, 161: 6, 222: 7}[K]
    A, B, A64, B64 = _operands(M, N, K, a_kc, b_kc, seed=K + 2 * a_kc + b_kc)
    bias = mask = None
    if epilogue:
        g = _gen(K)
        bias, mask = torch.randn(N, device="cuda", generator=g), torch.randn(M, N, device="cuda", generator=g)
    ref, yard, mag = _product(A64, B64, bias, epilogue, mask)
    got = gemm(A, B, a_kc, b_kc, bias=bias, relu=epilogue, mask=mask, terms=6)
    _check("1", "K=%d a_kc=%d b_kc=%d epilogue=%d" % (K, a_kc, b_kc, epilogue), got, ref, yard, mag)
    _report("1")


@gpu
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_item_stream_with_scaled_operands(a_kc, b_kc):
    """Group 1 at K = 161 with column k of A scaled by 2^e(k), e in [-20, 20], and row k of B by 2^-e(k): the products
    keep their values, the pieces of the operands do not keep their relative sizes. The elementwise bound must hold."""
    from egopose_amd.gemm import gemm
    M, N, K = 8000, 1664, 161
    assert _Plan(M, N, K).per_workgroup() >= 3
    e = torch.randint(-20, 21, (K,), device="cuda", generator=_gen(7))
    assert int(e.min()) == -20 and int(e.max()) == 20
    A, B, A64, B64 = _operands(M, N, K, a_kc, b_kc, seed=161, scale=torch.exp2(e.float()))
    ref, yard, mag = _product(A64, B64)
    _check("7", "a_kc=%d b_kc=%d" % (a_kc, b_kc), gemm(A, B, a_kc, b_kc, terms=6), ref, yard, mag)
    _report("7")


# ------------------------------------------------------------------------------ group 2: grid slots that hold no tile

@gpu
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("K", [95, 161])
def test_item_stream_with_empty_slots(a_kc, b_kc, K):
    """M = 8200: 65 row tiles, dealt to the XCDs in groups of 8 (xcd_order) and so padded to 72 -- 70 of the 720 grid slots
    hold no tile and the workgroups' streams skip them. With bias, into a column slice of a wider tensor (leading dimension
    1291, rows 4-byte aligned) whose other columns must keep their sentinel."""
    from egopose_amd.gemm import gemm
    M, N = 8200, 1280
    p = _Plan(M, N, K)
    assert p.xcd_order and p.tiles == 650 and p.slots == 720 and p.per_workgroup() >= 2
    A, B, A64, B64 = _operands(M, N, K, a_kc, b_kc, seed=K + 2 * a_kc + b_kc)
    bias = torch.randn(N, device="cuda", generator=_gen(K))
    ref, yard, mag = _product(A64, B64, bias)
    wide = torch.full((M, N + 11), SENTINEL, device="cuda")
    gemm(A, B, a_kc, b_kc, bias=bias, terms=6, out=wide[:, 3:3 + N])
    assert bool((wide[:, :3] == SENTINEL).all()) and bool((wide[:, 3 + N:] == SENTINEL).all()), "guard columns were written"
    _check("2", "K=%d a_kc=%d b_kc=%d" % (K, a_kc, b_kc), wide[:, 3:3 + N], ref, yard, mag)
    _report("2")


# ---------------------------------------------------------------------------------------- group 3: 64-column tiles

@gpu
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("N", [52, 64])
@pytest.mark.parametrize("K", [40, 95, 200])
def test_item_stream_64_column_tiles(a_kc, b_kc, N, K):
    """Outputs of at most 64 columns take 64-column tiles (one wave column, one MFMA block row per wave): M = 100 001 gives
    782 items, at least 3 per workgroup (M grows until that holds), in xcd_order with 2 empty slots."""
    from egopose_amd.gemm import gemm
    M = 100001
    while _Plan(M, N, K).per_workgroup() < 3:
        M += BM
    p = _Plan(M, N, K)
    assert p.bn == 64 and p.tiles_n == 1 and p.per_workgroup() >= 3 and p.ktiles == {40: 2, 95: 3, 200: 7}[K]
    A, B, A64, B64 = _operands(M, N, K, a_kc, b_kc, seed=N + K + 2 * a_kc + b_kc)
    ref, yard, mag = _product(A64, B64)
    _check("3", "N=%d K=%d a_kc=%d b_kc=%d" % (N, K, a_kc, b_kc), gemm(A, B, a_kc, b_kc, terms=6), ref, yard, mag)
    _report("3")


# ------------------------------------------------------------------- group 4: split-K past the CU count, remainder

def _wgrad_case(K, seed):
    g = _gen(seed)
    dy = torch.randn(K, 300, device="cuda", generator=g)
    x = torch.randn(K, 243, device="cuda", generator=g)
    return dy, x


def _check_wgrad(group, what, dW, db, dy, x, pre=None):
    """dW = dy^T x and db = column sums of dy against float64 (+ the prefilled `pre` = (out, bias_grad) when accumulating)."""
    A64, B64 = dy.double().t(), x.double()
    ref, yard, mag = _product(A64, B64)
    rb, yb, mb = A64.sum(1), dy.t().sum(1), A64.abs().sum(1)
    if pre is not None:
        ref, yard, mag = ref + pre[0].double(), yard + pre[0], mag + pre[0].double().abs()
        if db is not None:
            rb, yb, mb = rb + pre[1].double(), yb + pre[1], mb + pre[1].double().abs()
    _check(group, what + " dW", dW, ref, yard, mag, "split")
    if db is not None:
        _check(group, what + " db", db, rb, yb, mb, "split")


@gpu
@pytest.mark.parametrize("K,splits", [(20005, 128), (453, 8)])
def test_split_k_with_a_riding_remainder(K, splits, three_piece_kernel):
    """The update's dW shape (300 x 243 + the bias column, operands given as (K, M) and (K, N)). K = 20 005, splits = 128:
    ranges of 160 k rows, 126 of them, the last one 5 rows long -- shorter than a k-tile, so it rides with the range before it
    and k_gemm_ws writes 125 splits x 6 tiles = 750 items, more than there are CUs. K = 453, splits = 8: ranges of 64, a
    remainder of 5, 7 splits written. float64 agreement of dW and db, bit-identical repeats, accumulate into prefilled
    outputs."""
    from egopose_amd.gemm import gemm, usable_cus
    p = _Plan(300, 243, K, splits, ones=True)
    if K == 20005:
        assert (p.k_per_split, p.ranges, p.rem, p.written, p.items) == (160, 126, 5, 125, 750) and p.items > usable_cus()
    else:
        assert (p.k_per_split, p.ranges, p.rem, p.written) == (64, 8, 5, 7)
    assert p.rides and p.tiles == 6
    dy, x = _wgrad_case(K, seed=K)
    dW, db = gemm(dy, x, False, False, terms=6, splits=splits, want_bias_grad=True)
    assert dW.shape == (300, 243) and db.shape == (300,)
    _check_wgrad("4", "K=%d splits=%d" % (K, splits), dW, db, dy, x)
    for _ in range(2):
        dW2, db2 = gemm(dy, x, False, False, terms=6, splits=splits, want_bias_grad=True)
        assert torch.equal(dW, dW2) and torch.equal(db, db2), "fixed-order reduction: bit-identical from run to run"
    g = _gen(K + 1)
    pre = (torch.randn(300, 243, device="cuda", generator=g) * 50, torch.randn(300, device="cuda", generator=g) * 50)
    acc, accb = pre[0].clone(), pre[1].clone()
    gemm(dy, x, False, False, terms=6, splits=splits, want_bias_grad=True, out=acc, bias_grad_out=accb, accumulate=True)
    _check_wgrad("4", "K=%d splits=%d accumulate" % (K, splits), acc, accb, dy, x, pre)
    # the elementwise bound above cannot see a dropped addend of 50: that the product was added, not written, is exact
    assert torch.equal(acc, pre[0] + dW) and torch.equal(accb, pre[1] + db)
    _report("4")


@gpu
@pytest.mark.parametrize("K", [20005, 453])
def test_split_k_without_the_bias_column(K):
    """splits = 3 without the ones column (243 output columns: the partial sums go through 244-float workspace rows)."""
    from egopose_amd.gemm import gemm
    p = _Plan(300, 243, K, 3)
    assert p.ranges == 3 and not p.rides
    dy, x = _wgrad_case(K, seed=K + 3)
    dW = gemm(dy, x, False, False, terms=6, splits=3)
    _check_wgrad("4", "K=%d splits=3, no bias column" % K, dW, None, dy, x)
    assert torch.equal(dW, gemm(dy, x, False, False, terms=6, splits=3))
    _report("4")


@gpu
def test_split_k_after_a_larger_launch_on_the_same_workspace():
    """K = 453 / splits = 8 writes 7 of the workspace's split blocks right after a launch that filled 125 of them (same M and
    N, so the blocks coincide): the reduction must sum the 7 it was told about, not what the larger launch left behind."""
    from egopose_amd.gemm import gemm
    big, small = _wgrad_case(20005, seed=1), _wgrad_case(453, seed=2)
    assert _Plan(300, 243, 20005, 128, True).written > _Plan(300, 243, 453, 8, True).written == 7
    gemm(big[0], big[1], False, False, terms=6, splits=128, want_bias_grad=True)
    dW, db = gemm(small[0], small[1], False, False, terms=6, splits=8, want_bias_grad=True)
    _check_wgrad("4", "K=453 splits=8 after K=20005 splits=128", dW, db, *small)
    _report("4")


# ------------------------------------------------------------------------------------ group 5: gathers and scatters

def _indices(n, R, seed, repeats):
    """n row indices into a source of R > n rows. repeats: random with repeated entries, the last source row (and, from
    n = 4 on, the first one) among them. Otherwise distinct (a scatter's destination rows), first and last row included."""
    g = _gen(seed)
    if repeats:
        idx = torch.randint(0, R, (n,), device="cuda", generator=g)
        idx[0] = R - 1
        if n >= 4:
            idx[1], idx[n // 2], idx[n - 1] = 0, R - 1, idx[2]
    else:
        idx = torch.randperm(R - 2, device="cuda", generator=g)[:n] + 1
        idx[0], idx[n - 1] = R - 1, 0
    return idx.contiguous()


@gpu
@pytest.mark.parametrize("b_kc", [True, False])
@pytest.mark.parametrize("M", [1, 129, 4321])
def test_gathered_rows_of_a(M, b_kc, three_piece_kernel):
    """a_rows without a second source: row m of the operand is A[a_rows[m]], the indices repeat and include the first and the
    last row of a 5000-row source. float64 first, then bit for bit the product of the materialised operand."""
    from egopose_amd.gemm import gemm
    R, N, K = 5000, 300, 243
    g = _gen(M)
    src = torch.randn(R, K, device="cuda", generator=g)
    W = torch.randn(K, N, device="cuda", generator=g)
    B = W.t().contiguous() if b_kc else W
    idx = _indices(M, R, M, repeats=True)
    assert int(idx.max()) == R - 1 and (M < 4 or (int(idx.min()) == 0 and idx.unique().numel() < M))
    if three_piece_kernel == "classic":
        with pytest.raises(ValueError):
            gemm(src, B, True, b_kc, terms=6, a_rows=idx)
        return
    got = gemm(src, B, True, b_kc, terms=6, a_rows=idx)
    assert got.shape == (M, N)
    ref, yard, mag = _product(src.double().index_select(0, idx), W.double())
    _check("5", "a_rows M=%d b_kc=%d" % (M, b_kc), got, ref, yard, mag)
    assert torch.equal(got, gemm(src.index_select(0, idx).contiguous(), B, True, b_kc, terms=6))
    _report("5")


@gpu
@pytest.mark.parametrize("b_kc", [True, False])
@pytest.mark.parametrize("a_split", [32, 128])
@pytest.mark.parametrize("width", [32, 33, 115])
def test_gathered_rows_with_a_second_source(a_split, width, b_kc, three_piece_kernel):
    """a_rows + a2: columns [0, a_split) from the gathered source, the rest from a2, which is a column slice of a wider
    tensor (lda2 != width). Width 33: the last k-tile is read backwards from column 1 of a2."""
    from egopose_amd.gemm import gemm
    R, M, N = 3000, 777, 300
    g = _gen(a_split + width)
    src = torch.randn(R, a_split, device="cuda", generator=g)
    wide2 = torch.randn(M, width + 9, device="cuda", generator=g)
    a2 = wide2[:, 5:5 + width]
    W = torch.randn(a_split + width, N, device="cuda", generator=g)
    B = W.t().contiguous() if b_kc else W
    bias = torch.randn(N, device="cuda", generator=g)
    idx = _indices(M, R, width, repeats=True)
    if three_piece_kernel == "classic":
        with pytest.raises(ValueError):
            gemm(src, B, True, b_kc, terms=6, bias=bias, relu=True, a_rows=idx, a2=a2)
        return
    got = gemm(src, B, True, b_kc, terms=6, bias=bias, relu=True, a_rows=idx, a2=a2)
    x64 = torch.cat((src.double().index_select(0, idx), a2.double()), 1)
    ref, yard, mag = _product(x64, W.double(), bias, True)
    _check("5", "a_rows + a2, a_split=%d width=%d b_kc=%d" % (a_split, width, b_kc), got, ref, yard, mag)
    assert torch.equal(got, gemm(x64.float().contiguous(), B, True, b_kc, terms=6, bias=bias, relu=True))
    _report("5")


@gpu
@pytest.mark.parametrize("N", [52, 512])
def test_gather_and_scatter_into_a_column_slice(N, three_piece_kernel):
    """What the LSTM's row-list projection issues: a_rows + c_rows + bias into out[:, :N] of a wider prefilled tensor, on
    64-column tiles (N = 52) and on 128-column ones. Rows that no index names and the columns outside the slice keep their
    sentinel; the written rows agree with float64 and, bit for bit, with an index_copy of the unscattered product."""
    from egopose_amd.gemm import gemm
    R, M, K = 6000, 4500, 96
    g = _gen(N)
    src = torch.randn(R, K, device="cuda", generator=g)
    W = torch.randn(N, K, device="cuda", generator=g)
    bias = torch.randn(N, device="cuda", generator=g)
    rows = _indices(M, R, N, repeats=False)
    assert rows.unique().numel() == rows.numel() and int(rows.max()) == R - 1 and int(rows.min()) == 0
    out = torch.full((R, N + 24), SENTINEL, device="cuda")
    if three_piece_kernel == "classic":
        with pytest.raises(ValueError):
            gemm(src, W, True, True, terms=6, bias=bias, a_rows=rows, c_rows=rows, out=out[:, :N])
        return
    gemm(src, W, True, True, terms=6, bias=bias, a_rows=rows, c_rows=rows, out=out[:, :N])
    A64 = src.double().index_select(0, rows)
    ref, yard, mag = _product(A64, W.double().t(), bias)
    ref_out = torch.full((R, N + 24), SENTINEL, dtype=torch.float64, device="cuda")
    ref_out[rows, :N] = ref
    untouched = torch.ones(R, dtype=torch.bool, device="cuda")
    untouched[rows] = False
    assert int(untouched.sum()) == R - M
    assert torch.equal(out[:, N:].double(), ref_out[:, N:]), "columns outside the slice were written"
    assert torch.equal(out[untouched].double(), ref_out[untouched]), "rows that no index names were written"
    _check("5", "a_rows + c_rows + bias, N=%d" % N, out[rows, :N], ref_out[rows, :N], yard, mag)       # (the sentinel rows are exact, above)
    full = lambda t: torch.full((R, N), SENTINEL, device="cuda").index_copy_(0, rows, t)
    plain = gemm(src.index_select(0, rows).contiguous(), W, True, True, terms=6, bias=bias)
    assert torch.equal(out[:, :N], full(plain))
    _report("5")


@gpu
@pytest.mark.parametrize("N", [64, 128])
def test_scatter_with_mask(N, three_piece_kernel):
    """c_rows with the dReLU mask (mask rows follow the product's rows, not the destination's), B given as (K, N): the data
    gradient of a gathered first layer. 64- and 128-column tiles."""
    from egopose_amd.gemm import gemm
    R, M, K = 5000, 4321, 300
    g = _gen(N + 1)
    dz = torch.randn(M, K, device="cuda", generator=g)
    W = torch.randn(K, N, device="cuda", generator=g)
    maskw = torch.randn(M, N + 7, device="cuda", generator=g)
    mask = maskw[:, 2:2 + N]
    rows = _indices(M, R, N + 1, repeats=False)
    out = torch.full((R, N), SENTINEL, device="cuda")
    if three_piece_kernel == "classic":
        with pytest.raises(ValueError):
            gemm(dz, W, True, False, terms=6, mask=mask, out=out, c_rows=rows)
        return
    gemm(dz, W, True, False, terms=6, mask=mask, out=out, c_rows=rows)
    ref, yard, mag = _product(dz.double(), W.double(), mask=mask)
    ref_out = torch.full((R, N), SENTINEL, dtype=torch.float64, device="cuda")
    ref_out[rows] = ref
    untouched = torch.ones(R, dtype=torch.bool, device="cuda")
    untouched[rows] = False
    assert torch.equal(out[untouched].double(), ref_out[untouched]), "rows that no index names were written"
    _check("5", "c_rows + mask, N=%d" % N, out[rows], ref_out[rows], yard, mag)
    unscattered = gemm(dz, W, True, False, terms=6, mask=mask)
    assert torch.equal(out, torch.full((R, N), SENTINEL, device="cuda").index_copy_(0, rows, unscattered))
    _report("5")


@gpu
@pytest.mark.parametrize("M,N", [(512, 128), (52, 40), (300, 243)])
@pytest.mark.parametrize("K,splits", [(1005, 1), (1005, 7), (1005, 31), (965, 7), (965, 31)])
def test_gathered_k_rows_of_both_operands(M, N, K, splits, three_piece_kernel):
    """a_krows + b_krows: a weight gradient over K of the 5000 rows of its operands, in shuffled order (each operand with its
    own list). K = 1005: the last range ends 13 rows into a k-tile, which is read backwards (k0 = kend - 32) with its head
    zeroed. K = 965: the last range is 5 rows and rides with the one before it. 512 x 128 and 52 x 40 are the LSTM's dW
    shapes at small scale."""
    from egopose_amd.gemm import gemm
    R = 5000
    p = _Plan(M, N, K, splits, ones=True)
    if K == 965:
        assert p.rides and p.rem == 5 and p.written == (6 if splits == 7 else 30)
    else:
        assert not p.rides and p.rem % BK == 13 and p.ranges == {1: 1, 7: 7, 31: 16}[splits]
    g = _gen(M + K + splits)
    a_src = torch.randn(R, M, device="cuda", generator=g)
    b_src = torch.randn(R, N, device="cuda", generator=g)
    ka = torch.randperm(R, device="cuda", generator=g)[:K].contiguous()
    kb = torch.randperm(R, device="cuda", generator=g)[:K].contiguous()
    ka[K - 1], kb[0] = R - 1, R - 1
    kw = dict(terms=6, splits=splits, want_bias_grad=True)
    if three_piece_kernel == "classic":
        with pytest.raises(ValueError):
            gemm(a_src, b_src, False, False, a_krows=ka, b_krows=kb, **kw)
        return
    dW, db = gemm(a_src, b_src, False, False, a_krows=ka, b_krows=kb, **kw)
    assert dW.shape == (M, N) and db.shape == (M,)
    A64, B64 = a_src.double().index_select(0, ka).t(), b_src.double().index_select(0, kb)
    ref, yard, mag = _product(A64, B64)
    what = "a_krows + b_krows %dx%d K=%d splits=%d" % (M, N, K, splits)
    _check("5k", what + " dW", dW, ref, yard, mag, "split")
    _check("5k", what + " db", db, A64.sum(1), A64.float().sum(1), A64.abs().sum(1), "split")
    am, bm = a_src.index_select(0, ka).contiguous(), b_src.index_select(0, kb).contiguous()
    dW2, db2 = gemm(am, bm, False, False, **kw)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    if N % 4 == 0 and splits == 1:                          # a plain product (no workspace) with k-gathers
        got = gemm(a_src, b_src, False, False, terms=6, a_krows=ka, b_krows=kb)
        _check("5", what + " plain", got, ref, yard, mag)
        assert torch.equal(got, gemm(am, bm, False, False, terms=6))
    _report("5k")


@gpu
@pytest.mark.parametrize("width", [1, 4, 115])
def test_gathered_k_rows_with_a_second_source(width, three_piece_kernel):
    """b_krows + b2 + the bias column: the first layer's weight gradient reads [ctx[idx] | state] along k. Columns [0, 128) of
    B come from the gathered source, `width` columns from b2, then the ones column; width 1 leaves a second source of a
    single column."""
    from egopose_amd.gemm import gemm
    R, M, K, H, splits = 5000, 300, 1005, 128, 7
    g = _gen(width)
    dz = torch.randn(K, M, device="cuda", generator=g)
    ctx = torch.randn(R, H, device="cuda", generator=g)
    b2w = torch.randn(K + 1, width + 2, device="cuda", generator=g)
    b2 = b2w[:K, 1:1 + width]
    kb = torch.randperm(R, device="cuda", generator=g)[:K].contiguous()
    kw = dict(terms=6, splits=splits, want_bias_grad=True)
    if three_piece_kernel == "classic":
        with pytest.raises(ValueError):
            gemm(dz, ctx, False, False, b_krows=kb, b2=b2, **kw)
        return
    dW, db = gemm(dz, ctx, False, False, b_krows=kb, b2=b2, **kw)
    assert dW.shape == (M, H + width)
    A64 = dz.double().t()
    B64 = torch.cat((ctx.double().index_select(0, kb), b2.double()), 1)
    ref, yard, mag = _product(A64, B64)
    _check("5k", "b_krows + b2 width=%d dW" % width, dW, ref, yard, mag, "split")
    _check("5k", "b_krows + b2 width=%d db" % width, db, A64.sum(1), A64.float().sum(1), A64.abs().sum(1), "split")
    dW2, db2 = gemm(dz, B64.float().contiguous(), False, False, **kw)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    _report("5k")


@gpu
def test_gather_refusals_stay_refusals(three_piece_kernel):
    """A second source narrower than one k-tile, a second source of A with split-K, a scatter with split-K or with the bias
    column: ValueError, on either kernel."""
    from egopose_amd.gemm import gemm
    g = _gen(9)
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=g)
    src, a2, W = r(500, 128), r(400, 40), r(64, 168)
    idx = _indices(400, 500, 9, repeats=False)
    out = torch.zeros(500, 64, device="cuda")
    with pytest.raises(ValueError, match="a_split"):
        gemm(src, W[:, :148].contiguous(), True, True, terms=6, a_rows=idx, a2=a2[:, :20].contiguous())
    with pytest.raises(ValueError, match="A2 does not go with split-K"):
        gemm(src, W, True, True, terms=6, splits=2, a_rows=idx, a2=a2)
    with pytest.raises(ValueError, match="c_rows"):
        gemm(src, W[:, :128].contiguous(), True, True, terms=6, splits=2, a_rows=idx, c_rows=idx, out=out)
    with pytest.raises(ValueError, match="c_rows"):
        gemm(r(64, 400), r(64, 64), False, False, terms=6, want_bias_grad=True, c_rows=idx, out=out)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------ group 6: thin kernels

@gpu
@pytest.mark.parametrize("b_kc", [True, False])
@pytest.mark.parametrize("M", [1, 3, 4, 1025])
def test_gemv_rows(M, b_kc):
    """k_gemv_rows (N = 1, A given as (M, K)): four rows per workgroup and 64 lanes per row, so M = 1, 3, 4, 1025 and
    K = 1, 63, 64, 65, 243 cut both; B as (1, K) and as (K, 1); bias, ReLU and mask alone and together; strided out and mask."""
    from egopose_amd.gemm import gemm
    for K in (1, 63, 64, 65, 243):
        g = _gen(M + K)
        A = torch.randn(M, K, device="cuda", generator=g)
        w = torch.randn(K, 1, device="cuda", generator=g)
        B = w.t().contiguous() if b_kc else w
        bias = torch.randn(1, device="cuda", generator=g)
        maskw = torch.randn(M, 3, device="cuda", generator=g)
        for use_bias, relu, use_mask in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)]:
            b, m = (bias if use_bias else None), (maskw[:, 1:2] if use_mask else None)
            ref, yard, mag = _product(A.double(), w.double(), b, bool(relu), m)
            wide = torch.full((M, 3), SENTINEL, device="cuda")
            gemm(A, B, True, b_kc, bias=b, relu=bool(relu), mask=m, terms=6, out=wide[:, 1:2])
            assert bool((wide[:, 0] == SENTINEL).all()) and bool((wide[:, 2] == SENTINEL).all())
            _check("6", "gemv M=%d K=%d b_kc=%d bias=%d relu=%d mask=%d" % (M, K, b_kc, use_bias, relu, use_mask), wide[:, 1:2], ref, yard, mag,
                   "thin")
    _report("6")


@gpu
@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_rank1(a_kc, b_kc):
    """k_rank1 (K = 1) in the four layout combinations, 1 x 1, 5 x 243 and 1000 x 3, plain and with bias + ReLU + mask, into
    a column slice of a wider tensor."""
    from egopose_amd.gemm import gemm
    for M, N in ((1, 1), (5, 243), (1000, 3)):
        if N == 1 and a_kc:
            continue                                    # N = 1 with a k-contiguous A is k_gemv_rows' (test_gemv_rows, K = 1)
        A, B, A64, B64 = _operands(M, N, 1, a_kc, b_kc, seed=M + N)
        g = _gen(M * N)
        bias, mask = torch.randn(N, device="cuda", generator=g), torch.randn(M, N, device="cuda", generator=g)
        for epi in (False, True):
            ref, yard, mag = _product(A64, B64, bias if epi else None, epi, mask if epi else None)
            wide = torch.full((M, N + 5), SENTINEL, device="cuda")
            gemm(A, B, a_kc, b_kc, bias=bias if epi else None, relu=epi, mask=mask if epi else None, terms=6, out=wide[:, 2:2 + N])
            assert bool((wide[:, :2] == SENTINEL).all()) and bool((wide[:, 2 + N:] == SENTINEL).all())
            _check("6", "rank1 %dx%d a_kc=%d b_kc=%d epilogue=%d" % (M, N, a_kc, b_kc, epi), wide[:, 2:2 + N], ref, yard, mag, "thin")
    _report("6")


@gpu
@pytest.mark.parametrize("N", [1, 200, 256, 257, 600])
def test_colsum(N):
    """k_colsum (M = 1, A given as (K, 1), B as (K, N), split-K or the bias column): N past 256 runs its n0 loop, K = 1, 31,
    33 leave most of the 4 waves x 8 rows empty, splits > K gives one k row per workgroup; with and without the bias
    column, accumulate, bit-identical repeats."""
    from egopose_amd.gemm import gemm
    for K in (1, 31, 33, 9001):
        g = _gen(N + K)
        a = torch.randn(K, 1, device="cuda", generator=g)
        B = torch.randn(K, N, device="cuda", generator=g)
        ref, yard, mag = _product(a.double().t(), B.double())
        rb, yb, mb = a.double().sum(0), a.sum(0), a.double().abs().sum(0)
        for splits in (1, 7, 64, K + 3):
            what = "colsum N=%d K=%d splits=%d" % (N, K, splits)
            dW, db = gemm(a, B, False, False, terms=6, splits=splits, want_bias_grad=True)
            assert dW.shape == (1, N) and db.shape == (1,)
            _check("6", what + " dW", dW, ref, yard, mag, "thin")
            _check("6", what + " db", db, rb, yb, mb, "thin")
            dW2, db2 = gemm(a, B, False, False, terms=6, splits=splits, want_bias_grad=True)
            assert torch.equal(dW, dW2) and torch.equal(db, db2)
            if splits > 1:
                _check("6", what + " no bias column", gemm(a, B, False, False, terms=6, splits=splits), ref, yard, mag, "thin")
            pre = (torch.randn(1, N, device="cuda", generator=g) * 50, torch.randn(1, device="cuda", generator=g) * 50)
            acc, accb = pre[0].clone(), pre[1].clone()
            gemm(a, B, False, False, terms=6, splits=splits, want_bias_grad=True, out=acc, bias_grad_out=accb, accumulate=True)
            assert torch.equal(acc, pre[0] + dW) and torch.equal(accb, pre[1] + db)
    _report("6")


@gpu
@pytest.mark.parametrize("b_kc", [True, False])
def test_neighbours_of_the_thin_kernels(b_kc, three_piece_kernel):
    """M = 1 without split-K and N = 1 with A given as (K, M) are not thin-kernel shapes: a tiled kernel runs them (the
    profiler says so), to float32 class."""
    from egopose_amd.gemm import gemm
    thin = {"k_gemv_rows", "k_rank1", "k_colsum", "k_gemm_reduce"}
    A, B, A64, B64 = _operands(1, 200, 243, True, b_kc, seed=31)
    ref, yard, mag = _product(A64, B64)
    _check("6n", "M=1 N=200 K=243 b_kc=%d" % b_kc, gemm(A, B, True, b_kc, terms=6), ref, yard, mag)
    seen = _kernels_of(lambda: gemm(A, B, True, b_kc, terms=6))
    assert seen and not (seen & thin) and _tiled(three_piece_kernel)[0] in seen, seen
    A, B, A64, B64 = _operands(64, 1, 77, False, b_kc, seed=32)
    ref, yard, mag = _product(A64, B64)
    _check("6n", "M=64 N=1 K=77 A as (K, M) b_kc=%d" % b_kc, gemm(A, B, False, b_kc, terms=6), ref, yard, mag)
    seen = _kernels_of(lambda: gemm(A, B, False, b_kc, terms=6))
    assert seen == {"k_gemm_bf16x"}, seen               # (one column: no 16-byte rows for the persistent kernel)


# ------------------------------------------------------------------------------------------------- dispatch check

@gpu
def test_profiler_sees_the_expected_kernels(three_piece_kernel):
    """One case of every group under torch.profiler: the kernel the group is about runs and the others do not."""
    from egopose_amd.gemm import gemm
    tiled, other = _tiled(three_piece_kernel)
    ws = three_piece_kernel == "ws"
    g = _gen(77)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)

    A, B = r(8000, 95), r(1664, 95)
    assert _kernels_of(lambda: gemm(A, B, terms=6)) == {tiled}                                             # group 1 (and 7)
    A, B, bias, wide = r(8200, 95), r(1280, 95), r(1280), r(8200, 1291)
    assert _kernels_of(lambda: gemm(A, B, terms=6, bias=bias, out=wide[:, 3:1283])) == {tiled}              # group 2
    A, B = r(100001, 40), r(52, 40)
    assert _kernels_of(lambda: gemm(A, B, terms=6)) == {tiled}                                             # group 3
    dy, x = _wgrad_case(453, 5)
    assert _kernels_of(lambda: gemm(dy, x, False, False, terms=6, splits=8, want_bias_grad=True)) == {tiled, "k_gemm_reduce"}     # group 4
    dy, x = _wgrad_case(20005, 5)
    assert _kernels_of(lambda: gemm(dy, x, False, False, terms=6, splits=128, want_bias_grad=True)) == {tiled, "k_gemm_reduce"}
    if ws:                                                                                                  # group 5
        src, W, idx = r(5000, 243), r(300, 243), _indices(4321, 5000, 1, repeats=True)
        assert _kernels_of(lambda: gemm(src, W, terms=6, a_rows=idx)) == {"k_gemm_ws"}
        a_src, b_src = r(5000, 512), r(5000, 128)
        ka = torch.randperm(5000, device="cuda", generator=g)[:965].contiguous()
        assert _kernels_of(lambda: gemm(a_src, b_src, False, False, terms=6, splits=7, want_bias_grad=True, a_krows=ka, b_krows=ka)) \
            == {"k_gemm_ws", "k_gemm_reduce"}
        dz, W2, rows, out = r(4321, 300), r(300, 128), _indices(4321, 5000, 2, repeats=False), torch.zeros(5000, 128, device="cuda")
        assert _kernels_of(lambda: gemm(dz, W2, True, False, terms=6, out=out, c_rows=rows)) == {"k_gemm_ws"}
    A, w = r(1025, 243), r(1, 243)                                                                           # group 6
    assert _kernels_of(lambda: gemm(A, w, terms=6, relu=True)) == {"k_gemv_rows"}
    a, b = r(5, 1), r(243, 1)
    assert _kernels_of(lambda: gemm(a, b, terms=6)) == {"k_rank1"}
    a, B = r(9001, 1), r(9001, 600)
    assert _kernels_of(lambda: gemm(a, B, False, False, terms=6, splits=64, want_bias_grad=True)) == {"k_colsum", "k_gemm_reduce"}
    assert _kernels_of(lambda: gemm(a, B, False, False, terms=6, want_bias_grad=True)) == {"k_colsum", "k_gemm_reduce"}


# ------------------------------------------------------------------------------------------- the accumulate gap

@gpu
def test_accumulate_on_a_plain_product_is_refused():
    """accumulate reaches only the split-K reduction: on a plain product (splits = 1, no bias gradient) the epilogue would
    overwrite `out`. gemm() refuses it and so does egp_gemm_f32 (EGP_E_INVALID, `out` untouched)."""
    import ctypes as C
    from egopose_amd import _lib as L
    from egopose_amd.gemm import gemm
    g = _gen(6)
    A, B = torch.randn(200, 64, device="cuda", generator=g), torch.randn(128, 64, device="cuda", generator=g)
    out = torch.full((200, 128), SENTINEL, device="cuda")
    with pytest.raises(ValueError):
        gemm(A, B, terms=6, out=out, accumulate=True)
    with pytest.raises(ValueError):
        gemm(A, B, terms=6, out=out, accumulate=True, bias=torch.zeros(128, device="cuda"))
    d = L.GemmDesc()
    d.M, d.N, d.K = 200, 128, 64
    d.A, d.lda, d.a_kcontig = A.data_ptr(), 64, 1
    d.B, d.ldb, d.b_kcontig = B.data_ptr(), 64, 1
    d.C, d.ldc = out.data_ptr(), 128
    d.terms, d.splits, d.accumulate = 6, 1, 1
    lib = L.load()
    rc = lib.egp_gemm_f32(C.byref(d), L.current_stream())
    assert rc != 0 and b"accumulate" in lib.egp_last_error()
    with pytest.raises(ValueError):
        L.check(rc, "egp_gemm_f32")
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    d.accumulate = 0
    L.check(lib.egp_gemm_f32(C.byref(d), L.current_stream()), "egp_gemm_f32")
    assert _rel(out, A.double() @ B.double().t()) < 1e-6
    # where it is documented it stays: split-K and bias-gradient launches add
    dy, x = _wgrad_case(453, 4)
    acc, accb = torch.ones(300, 243, device="cuda"), torch.ones(300, device="cuda")
    dW, db = gemm(dy, x, False, False, terms=6, want_bias_grad=True)
    gemm(dy, x, False, False, terms=6, want_bias_grad=True, out=acc, bias_grad_out=accb, accumulate=True)
    assert torch.equal(acc, 1 + dW) and torch.equal(accb, 1 + db)


# ------------------------------------------------------------------- self-check of the tolerances (CPU, float64 only)

def _truncate16(a64):
    """float32 values cut to 16 mantissa bits (two bf16 pieces): the third piece lost."""
    a = a64.float()
    hi = (a.view(torch.int32) & -65536).view(torch.float32)
    r = a - hi
    mid = (r.view(torch.int32) & -65536).view(torch.float32)
    return (hi + mid).double()


def test_tolerance_tells_a_wrong_answer():
    """With the float64 reference and the float32 yardstick alone (CPU): each modelled fault misses the tolerance of its
    group by at least SELF_MARGIN."""
    margins = {}
    # groups 1-3, 7 (direct products): a case of group 1 cut to 2 x 2 tiles, K = 95 (3 k-tiles, the last read backwards)
    M, N, K = 256, 256, 95
    _, _, A64, B64 = _operands(M, N, K, True, True, seed=1, device="cpu")
    ref, yard, mag = _product(A64, B64)
    margins["a direct"] = _margin(_truncate16(A64) @ B64, ref, yard, mag, "direct")
    kbeg, kend, nst = 0, K, -(-K // BK)
    lo, hi = kend - BK, kbeg + BK * (nst - 1)
    assert lo < hi
    wrong = ref.clone()
    wrong[:BM] += A64[:BM, lo:hi] @ B64[lo:hi]
    margins["b direct"] = _margin(wrong, ref, yard, mag, "direct")
    wrong = ref.clone()
    wrong[:BM, :128] = ref[:BM, 128:256]
    margins["c direct"] = _margin(wrong, ref, yard, mag, "direct")
    # group 4 (split-K): the K = 453 / splits = 8 case, ranges of 64 k rows; the tail tile of the last written range
    K = 453
    g = _gen(2, "cpu")
    dy, x = torch.randn(K, 300, generator=g), torch.randn(K, 243, generator=g)
    A64, B64 = dy.double().t(), x.double()
    ref, yard, mag = _product(A64, B64)
    margins["a split"] = _margin(_truncate16(A64) @ B64, ref, yard, mag, "split")
    p = _Plan(300, 243, K, 8, ones=True)
    kbeg, kend = (p.written - 1) * p.k_per_split, K
    nst = -(-(kend - kbeg) // BK)
    lo, hi = kend - BK, kbeg + BK * (nst - 1)
    assert p.rides and lo < hi
    wrong = ref.clone()
    wrong[:BM] += A64[:BM, lo:hi] @ B64[lo:hi]
    margins["b split"] = _margin(wrong, ref, yard, mag, "split")
    wrong = ref.clone()
    wrong[:BM, :115] = ref[BM:2 * BM, 128:243]
    margins["c split"] = _margin(wrong, ref, yard, mag, "split")
    # group 5: a gather (a_rows) and a scatter (c_rows) with one index off by one row
    R, M, N, K = 500, 300, 64, 96
    g = _gen(3, "cpu")
    src, W = torch.randn(R, K, generator=g).double(), torch.randn(K, N, generator=g).double()
    idx = torch.randperm(R, generator=g)[:M]
    idx[7] = 100
    ref, yard, mag = _product(src[idx], W)
    off = idx.clone()
    off[7] += 1
    margins["d gather"] = _margin(src[off] @ W, ref, yard, mag, "direct")
    margins["a gather"] = _margin(_truncate16(src[idx]) @ W, ref, yard, mag, "direct")
    full = lambda t, rows, fill: torch.full((R, N), fill, dtype=t.dtype).index_copy_(0, rows, t)
    idx = torch.randperm(R - 1, generator=g)[:M]
    off = idx.clone()
    off[7] = R - 1                                      # (a free row: the shifted scatter leaves row idx[7] unwritten)
    margins["d scatter"] = _margin(full(ref, off, SENTINEL), full(ref, idx, SENTINEL), full(yard, idx, SENTINEL), full(mag, idx, 1.0), "direct")
    # group 6 (thin): a gemv with a truncated operand, and a column sum that takes a neighbour's column
    A64, w64 = torch.randn(1025, 243, generator=g).double(), torch.randn(243, 1, generator=g).double()
    ref, yard, mag = _product(A64, w64)
    margins["a thin"] = _margin(_truncate16(A64) @ w64, ref, yard, mag, "thin")
    wrong = ref.clone()
    wrong[4:8] = ref[0:4]
    margins["c thin"] = _margin(wrong, ref, yard, mag, "thin")
    print("\n  self-check margins: " + ", ".join("%s %.0fx" % kv for kv in sorted(margins.items())))
    low = {k: v for k, v in margins.items() if not v >= SELF_MARGIN}
    assert not low, low


def test_plan_matches_the_issue_arithmetic():
    """The launcher's arithmetic as this file restates it, at the figures the cases rely on (no GPU needed)."""
    p = _Plan(300, 243, 20005, 128, ones=True)
    assert (p.k_per_split, p.ranges, p.rem, p.rides, p.written, p.items) == (160, 126, 5, True, 125, 750)
    p = _Plan(300, 243, 453, 8, ones=True)
    assert (p.k_per_split, p.ranges, p.rem, p.rides, p.written) == (64, 8, 5, True, 7)
    p = _Plan(8200, 1280, 95)
    assert (p.tiles_m, p.tiles, p.slots, p.xcd_order) == (65, 650, 720, True)
    p = _Plan(8000, 1664, 222)
    assert (p.tiles, p.slots, p.xcd_order, p.ktiles) == (819, 819, False, 7)
    assert _Plan(100001, 52, 40).bn == 64 and _Plan(100001, 65, 40).bn == 128 and math.ceil(100001 / BM) == 782
