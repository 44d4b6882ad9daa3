"""Cases and data of the exact tests of the large-tile bf16 GEMMs (tests/test_hip_gemm_large_exact.py runs them on the GPU,
tests/test_gemm_large_host.py asserts the rules below for every one of them on the CPU, through `host_cases()`).

Data rules
  Integer operands.  Every partial sum is an integer below 2^24, so the fp32 accumulators hold the fp64 product in any order
    (`gemm_small_ref.expected` asserts the range) and the assertion on the GPU is EQUALITY.
  Unit sensitivity.  A bf16 store rounds to 8 significant bits, so a sum that is off by one shows only where a bf16 step is
    at most 1: every value v at a rounding point of a bf16-output equality case satisfies bf16(v + 1) != bf16(v) and
    bf16(v - 1) != bf16(v), i.e. |v| <= 255 (`rounding_points`, `unit_sensitive`).  The operands that keep the sums there:
      K <= 320   a, w of [-2, 2]                                          (sigma of a sum <= 36)
      K >  320   w of {-1, 0, 1}, a of {-1, 0, 1} with half its entries zeroed  (sigma <= 38 at K = 6400)
    and for the gated forms, whose factor 2 doubles the sum in front of the last rounding ("tight" data):
      K <= 320   a, w of {-1, 0, 1};   K > 320: a keeps min(1/2, 560 / K) of its entries  (sigma <= 16)
    with a bias of [-4, 4] and a residual of [-32, 32] (tight: [-16, 16]).
  Gates are the exact powers of two {+-0.5, +-1, +-2}, gate[b, n] = VALUES[(n + b + s) % 6]: the gates of neighbouring batches
    and of neighbouring columns (and of columns 8, 128 or 256 apart) differ.  Neither gate * bf16(y) nor its sum with the
    residual rounds (`gate_is_exact`), so one wrong product moves the stored value by |gate| and a gate from the wrong batch
    or column changes every element whose y is not 0.
  Per problem.  W, the bias and the gate's offset s are seeded by M too, so the problems of a grouped launch, which share
    (N, K), have no bias, W row or gate row in common: a tile that reads them through the wrong problem index stores other bits.
  K padding.  A and W are the views [:, :K] of buffers with K + 16 columns whose last 16 hold NaN (lda = ldw = K + 16): a
    read past K turns the output into NaN.
  GELU / SiLU cases scale w by a power of two so that |y| <= 8; they are held to 1 bf16 ulp, not to equality, and the unit
    sensitivity rule does not speak about them.

Launch forms: 128 = gemm9 (256 x 128), 256 = gemm8, 384 = gemm_mix, 512 = split-K pairs, 640 = stream-K ranges, 1024 = gemm10
(16 x 16 x 32 MFMA only).  A case whose forced form does not apply is a mistake in these tables.

Section W (tests/test_hip_gemm_walk_exact.py): forms 256 and 384 as the tile walk, every launch under the workgroup caps of
`walk_caps`.  The same data rules through the same `case_problem`; what the launcher decides for a mixed grid (`mixed_big_cols`)
and the order in which a workgroup meets big and small tiles (`mix_table`, `mix_place`, `walk_shapes`) are restated here and held
against csrc/gemm_tile_map.h by tests/test_gemm_large_host.py.
"""
import functools
import math

import torch

import gemm_small_ref as R
from gemm_small_ref import BF, F32, F64

PAD = 16
GATE_VALUES = (0.5, -1.0, 2.0, -0.5, 1.0, -2.0)
ALPHAS = {"scale_pow2": 0.125, "scale_rsqrt512": 512 ** -0.5}
EPILOGUES = ("none_bias", "none", "scale_pow2", "scale_rsqrt512", "res", "res_inplace", "gelu", "silu", "gate_res",
             "gate_res_inplace")                       # test_hip_gemm_small.py's FORMS_2D + FORMS_GATE
GATED = ("gate_res", "gate_res_inplace")
ACTIVATIONS = ("gelu", "silu")
MFMA_OF = {128: (16, 32), 256: (16, 32), 384: (16, 32), 512: (16, 32), 640: (16, 32), 1024: (16,)}
SK_MIN_PART = 16          # csrc/gemm_pingpong_bf16.hip: the shortest part of a tile's K range a stream-K cut may leave

# ---- the sections' tables -----------------------------------------------------------------------------------------------------
A_KS = (64, 128, 192, 256, 320)                        # 1 .. 5 K-tiles: prologue only, one trip, odd exit, two trips, odd again
A_MS = (192, 255, 256, 257, 300, 513)
A_SHAPES = {128: [(M, N) for M in A_MS for N in (8, 136, 392, 768)],
            256: [(M, N) for M in A_MS for N in (256, 768)],
            1024: [(M, N) for M in A_MS for N in (256, 768)],
            384: [(M, N) for M in (257, 300, 513) for N in (768, 1024)]}
B_KS = (64, 192)
B_SHAPES = {128: [(300, 392)], 256: [(300, 768), (513, 256)], 384: [(300, 768)], 1024: [(300, 768), (513, 256)]}
C_BR = ((2, 150), (4, 70), (5, 60), (3, 85), (2, 127), (2, 128), (2, 129), (2, 255), (2, 257), (300, 1))
C_N, C_K, C_S_TXT = 512, 128, 10
C_FORMS = (128, 256, 1024)
C_EPILOGUES = ("none_bias", "res_inplace", "gate_res", "gate_res_inplace")
D_BR = ((1, 1), (2, 150), (3, 700), (1, 257))           # M = 1, 300, 2100, 257 in one call
D_N, D_K = 512, 192
D_FORMS = (128, 256, 1024)
D_EPILOGUES = ("none_bias", "gate_res")
D_GROUP_M = (0, 1, 3)
E_KS = (256, 512, 768, 6144, 6400)                      # halves of 2, 4, 6, 48 and 50 K-tiles
E_SHAPES = ((256, 256), (300, 512), (513, 256))         # 1, 4 and 3 tiles
E_EXCHANGES = ("symmetric", "whole", "unannounced")      # named, not "default": whatever the library was built with
E_EPILOGUES = ("f32", "none_bias", "res_inplace", "gate_res", "gelu")
E_GATE_BR = (2, 150)
E_SEQUENCE = [((256, 256), (300, 256), (513, 512))[i % 3] + ((256, 768)[i % 2],) for i in range(20)]   # 1, 2 and 6 tiles
F_SLOTS = (2, 3, 4, 5)
F_KS = (2048, 3072, 6400)
F_EPILOGUES = ("f32", "none_bias", "gate_res")
G_KS = (64, 192)
G_EPILOGUES = ("f32", "none_bias", "gate_res")
# section W: the tile walk (gemm_walk_kernel) under workgroup caps, tests/test_hip_gemm_walk_exact.py.  It reuses the tables of
# A .. D at forms 256 / 384 (bf16 output: the walk has no fp32-parity epilogue) and adds:
W_FORMS = (256, 384)
W_EPI_A = "none_bias"
W_LONG_KS = (3072, 6144, 6400)                          # 48, 96 and 100 K-tiles: even and odd trip counts at production depth
W_LONG_SHAPES = {256: (513, 768), 384: (513, 1024)}     # 9 tiles; 3 big + 18 small
W_C_FORM = W_D_FORM = 256
W_GM_BR = ((2, 150), (4, 130), (1, 257))                # the mixed form's grouped case: M = 300, 520, 257, 2 + 3 + 2 row tiles
W_GM_N, W_GM_K = 768, 192
W_GM_GROUP_M = (0, 2)
W_H_BATCH, W_H_S_TXT, W_H_S_IMG, W_H_HEADS = 2, 70, 280, 2   # section H's shapes (its data is random, not from `problem`)
W_H_THIRDS = (3, 2)
FK_RATE_256 = 1.22        # csrc/gemm_pingpong_bf16.hip: rate of the 256 x 256 kernel over the 256 x 128 one in the launch plan


def tiles256(M, N):
    return -(-M // 256) * -(-N // 256)


def e_applies(M, N, K, epi):
    """Which (shape, K, epilogue) combinations section E runs: the gated form at (2, 150), GELU at the short K."""
    if epi == "gate_res":
        return M == E_GATE_BR[0] * E_GATE_BR[1]
    if epi == "gelu":
        return K <= 768
    return True


def cut_kinds(tiles, nk, grid, min_part=SK_MIN_PART):
    """`cut()` of gemm8_streamk_kernel restated: cut j of `grid` equal ranges over tiles x nk K-tiles lies at floor(U j / G);
    a cut that would leave a part shorter than `min_part` K-tiles moves onto the tile boundary behind or in front of it.
    Returns ([position of cut 1 .. G - 1], [kind]) with kind one of boundary / back / forward / in_place."""
    U = tiles * nk
    pos, kinds = [], []
    for j in range(1, grid):
        c = U * j // grid
        r = c % nk
        if r == 0:
            kinds.append("boundary")
        elif r < min_part:
            kinds.append("back")
            c -= r
        elif nk - r < min_part:
            kinds.append("forward")
            c += nk - r
        else:
            kinds.append("in_place")
        pos.append(c)
    return pos, kinds


@functools.lru_cache(maxsize=None)
def streamk_cases():
    """(slots, M, N, K) of section F: the smallest grid the forced form takes, tiles x nk >= slots x (nk + 2 min_part), as
    row tiles x 1, 2 or 3 column tiles with a ragged last row tile; M is even (the gated form runs it as two batches)."""
    out = []
    for K in F_KS:
        nk = K // 64
        for slots in F_SLOTS:
            t = -(-slots * (nk + 2 * SK_MIN_PART) // nk)
            cols = next(c for c in (2, 3, 1) if t % c == 0 and t // c >= 2)      # at least two row tiles: M >= 192
            M, N = 256 * (t // cols) - 212, 256 * cols
            assert tiles256(M, N) == t and M % 2 == 0 and t * nk >= slots * (nk + 2 * SK_MIN_PART) > (t - 1) * nk
            out.append((slots, M, N, K))
    return out


def persistent_grid(cus):
    """Section G: (M, N, B, R) of the smallest square-ish grid of >= 4 x CUs tiles, one column tile more than row tiles so the
    workgroups walk unequal tile counts, the last row tile ragged.  256 CUs: 32 x 33 tiles, M = 8092 = 28 x 289, N = 8448."""
    rt = math.isqrt(4 * cus - 1) + 1
    M, N = 256 * rt - 100, 256 * (rt + 1)
    B = 28 if M % 28 == 0 else 4
    assert tiles256(M, N) >= 4 * cus and M % 256 != 0 and M % B == 0
    return M, N, B, M // B


# ---- section W: the caps, and the launcher's mixed grid and its place order restated ------------------------------------------

def walk_caps(tiles):
    """The caps (workgroups of the launch) a launch of `tiles` places runs under: 1 (one workgroup walks the whole launch, the
    longest chain of hand-overs), 2, 3 and tiles - 1 (tiles == cap + 1: workgroup 0 alone is handed a second tile), each only
    where tiles > cap -- at tiles <= cap the launcher keeps one workgroup per tile -- and once.  A one-tile launch gets none."""
    out = []
    for cap in (1, 2, 3, tiles - 1):
        if 1 <= cap < tiles and cap not in out:
            out.append(cap)
    return out


def makespan(nb, ns, cs, G):
    """`makespan()` of csrc/gemm_pingpong_bf16.hip restated: nb tiles of cost 1, then ns of cost cs, list-scheduled on G CUs."""
    full, rem = divmod(nb, G)
    ta, tb = float(full), float(full) + 1.0
    end = 0.0 if nb == 0 else (tb if rem else ta)
    na = G - rem
    while ns > 0:
        if rem == 0 or ta <= tb:
            ta, ns = ta + cs, ns - min(ns, na)
            end = max(end, ta)
        else:
            tb, ns = tb + cs, ns - min(ns, rem)
            end = max(end, tb)
    return end


def mixed_big_cols(nbm, N, cus=256):
    """Column tiles of 256 in the mixed grid that the forced form 384 launches for `nbm` row tiles (summed over the problems)
    of width N on `cus` CUs -- fk_gemm2_launch restated: the launch plan's own split where a mixed grid pays, else the split
    of the shortest makespan (the first of equals) among those with at least 8 small tiles; 0: the form does not apply."""
    if N % 256 != 0 or N < 512:
        return 0
    c128, nb256 = 0.5 * FK_RATE_256, N // 256
    tbest = min(makespan(0, nbm * (N // 128), c128, cus), makespan(nbm * nb256, 0, c128, cus))
    splits = [cb for cb in range(1, nb256) if nbm * 2 * (nb256 - cb) >= 8]
    planned = 0
    for cb in splits:
        t = makespan(nbm * cb, nbm * 2 * (nb256 - cb), c128, cus)
        if t < tbest * 0.97:
            tbest, planned = t, cb
    if planned:
        return planned
    forced, tb = 0, 1e30
    for cb in splits:
        t = makespan(nbm * cb, nbm * 2 * (nb256 - cb), c128, cus)
        if t < tb:
            tb, forced = t, cb
    return forced


def walk_grid(form, Ms, N, cus=256):
    """(big tiles, small tiles) of the launch of problems with rows `Ms` and width N under form 256 (no small ones) / 384."""
    nbm = sum(-(-M // 256) for M in Ms)
    if form == 256:
        return nbm * (N // 256), 0
    cb = mixed_big_cols(nbm, N, cus)
    assert form == 384 and cb > 0, f"the mixed form does not apply to Ms {Ms} N {N}"
    return nbm * cb, nbm * 2 * (N // 256 - cb)


def mix_table(tb, ts):
    """`tm_fill_mix()` of csrc/gemm_tile_map.h restated: per XCD (first big tile, big tiles, first small tile); None where an
    XCD would get fewer places than big tiles (the launcher then falls back to a plain grid)."""
    W, table, bs, ss = tb + ts, [], 0, 0
    for x in range(8):
        wx, bx = W // 8 + (x < W % 8), tb // 8 + (x < tb % 8)
        if wx < bx:
            return None
        table.append((bs, bx, ss))
        bs, ss = bs + bx, ss + wx - bx
    return table


def mix_place(table, b):
    """`tm_mix_place()` restated: place b of a mixed launch is (small, tile index inside its class)."""
    big_start, big_cnt, small_start = table[b & 7]
    idx = b >> 3
    return (True, small_start + idx - big_cnt) if idx >= big_cnt else (False, big_start + idx)


def walk_shapes(tb, ts, cap):
    """The tile walk's place order restated (tm_walk_count / tm_walk_place): for each of the min(cap, places) workgroups the
    shapes (True: 256 x 128) of its places g, g + cap, ... in turn.  A pure grid (ts == 0) has big tiles only."""
    places = tb + ts
    table = mix_table(tb, ts) if ts else None
    assert not ts or table is not None
    return [[bool(ts) and mix_place(table, b)[0] for b in range(g, places, cap)] for g in range(min(cap, places))]


def shape_changes(tb, ts, cap):
    """Hand-overs of a launch under `cap` that change the tile shape: (the most inside one workgroup's list, big -> small ones
    in all, small -> big ones in all).  Each of them takes the workgroup barrier in `hand_over` of gemm_walk_kernel."""
    most = to_small = to_big = 0
    for shapes in walk_shapes(tb, ts, cap):
        ch = [(a, b) for a, b in zip(shapes, shapes[1:]) if a != b]
        most = max(most, len(ch))
        to_small += sum(1 for a, b in ch if b)
        to_big += sum(1 for a, b in ch if not b)
    return most, to_small, to_big


def w_h_problems():
    """Rows of the two problems of section H's grouped launch (image rows of both batches, text rows) and its widths."""
    return (W_H_BATCH * W_H_S_IMG, W_H_BATCH * W_H_S_TXT), [t * W_H_HEADS * 128 for t in W_H_THIRDS]


def walk_launches():
    """Sorted unique (part, form, rows of the problems, N, K) of every launch shape of section W, one-tile launches (which get
    no cap) left out: what tests/test_hip_gemm_walk_exact.py runs under each cap of `walk_caps(sum(walk_grid(...)))`."""
    out = set()
    for form in W_FORMS:
        out |= {("A", form, (M,), N, K) for M, N in A_SHAPES[form] for K in A_KS}
        out |= {("A", form, (W_LONG_SHAPES[form][0],), W_LONG_SHAPES[form][1], K) for K in W_LONG_KS}
        out |= {("B", form, (M,), N, K) for M, N in B_SHAPES[form] for K in B_KS}
        out |= {("H", form, w_h_problems()[0], N, 192) for N in w_h_problems()[1]}
    out |= {("C", W_C_FORM, (B * Rr,), C_N, C_K) for B, Rr in C_BR}
    out.add(("D", W_D_FORM, tuple(B * Rr for B, Rr in D_BR), D_N, D_K))
    out.add(("D", 384, tuple(B * Rr for B, Rr in W_GM_BR), W_GM_N, W_GM_K))
    return sorted(c for c in out if sum(walk_grid(c[1], c[2], c[3])) > 1)


# ---- data -----------------------------------------------------------------------------------------------------------------------

def nan_padded(x):
    """(buffer [rows, K + PAD] with NaN in its last PAD columns, its view [:, :K])."""
    rows, K = x.shape
    full = torch.full((rows, K + PAD), float("nan"), dtype=BF)
    full[:, :K] = x
    return full, full[:, :K]


def operands(M, N, K, tight):
    """(a [M, K], w [N, K]) by the rules of the module docstring."""
    s = 17 * M + 31 * N + K + (7919 if tight else 0)
    if K <= 320:
        lim = 1 if tight else 2
        return R.ints((M, K), -lim, lim, 100000 + s), R.ints((N, K), -lim, lim, 200000 + s)
    a, w = R.ints((M, K), -1, 1, 100000 + s), R.ints((N, K), -1, 1, 200000 + s)
    keep = min(0.5, 560.0 / K) if tight else 0.5
    mask = torch.rand((M, K), generator=torch.Generator().manual_seed(300000 + s)) < keep
    return (a.float() * mask).to(BF), w


def gate_seed(M, K):
    """Offset of a problem's gate pattern: distinct modulo 6 for the problems of a grouped launch (M = 1, 300, 2100, 257 at one K),
    so at every batch index their gate rows differ in every column."""
    return M + 3 * (M // 256) + K


def gates(B, N, seed):
    """[B, 3 N] bf16 whose columns [N, 2 N) are the gate: VALUES[(n + b + seed) % 6]; the other two thirds hold 3 (no gate value)."""
    idx = (torch.arange(N)[None] + torch.arange(B)[:, None] + seed) % len(GATE_VALUES)
    wide = torch.full((B, 3 * N), 3.0, dtype=BF)
    wide[:, N:2 * N] = torch.tensor(GATE_VALUES, dtype=BF)[idx]
    return wide


class Problem:
    """Inputs and the exact product of one shape (never modified).  B: batches of the gate; tight: data of the gated forms."""

    def __init__(self, M, N, K, B=1, tight=False):
        self.M, self.N, self.K, self.B, self.tight = M, N, K, B, tight
        a, w = operands(M, N, K, tight)
        (self.a_full, self.a), (self.w_full, self.w) = nan_padded(a), nan_padded(w)
        self.bias = R.ints((N,), -4, 4, 400000 + 7 * M + N + K)      # by M too: the problems of a grouped launch share (N, K)
        lim = 16 if tight else 32
        self.res = R.ints((M, N), -lim, lim, 500000 + M + N)
        self.gate_wide = gates(B, N, gate_seed(M, K))
        self.gate = self.gate_wide[:, N:2 * N]
        self._y0 = self._act = None

    @property
    def y0(self):
        if self._y0 is None:
            self._y0 = R.expected(self.a, self.w)
        return self._y0

    def sample(self, rows, rows_per_batch):
        """The same problem restricted to the rows `rows` (a LongTensor), as a problem of one row per batch: every sampled
        row keeps its own gate row, so the predicates below apply with rows_per_batch = 1.  For the CPU checks of the one
        large problem (section G), which then never form the whole product."""
        S = object.__new__(Problem)
        S.M, S.N, S.K, S.B, S.tight = len(rows), self.N, self.K, len(rows), self.tight
        (S.a_full, S.a), (S.w_full, S.w) = nan_padded(self.a[rows]), (self.w_full, self.w)
        S.bias, S.res = self.bias, self.res[rows]
        S.gate_wide = self.gate_wide[rows // rows_per_batch]
        S.gate = S.gate_wide[:, self.N:2 * self.N]
        S._y0 = S._act = None
        return S

    @property
    def y(self):
        return R.expected(self.a, self.w, self.bias, product=self.y0)

    @property
    def act(self):
        """(w_act_full, y_act): w times the largest power of two that keeps |a w^T| <= 4, so |y| <= 8 with the bias."""
        if self._act is None:
            s = 2.0 ** math.floor(math.log2(4.0 / max(self.y0.abs().max().item(), 1.0)))
            w_act = (self.w.float() * s).to(BF)
            assert torch.equal(w_act.float(), self.w.float() * s)
            full, view = nan_padded(w_act)
            y_act = R.expected(self.a, view, self.bias)
            assert y_act.abs().max().item() <= 8
            self._act = (full, y_act)
        return self._act


problem = functools.lru_cache(maxsize=None)(Problem)
big_problem = functools.lru_cache(maxsize=1)(Problem)        # section G: half a gigabyte of fp64 each, one at a time


def want(epi, P, rows_per_batch=None):
    """(the output the kernel must store, "eq" / "ulp") of epilogue `epi` ("f32": the fp32 build with bias) on problem P."""
    if epi == "f32":
        return R.f32_none(P.y0, P.bias), "eq"
    if epi == "none_bias":
        return R.epi_none(P.y), "eq"
    if epi == "none":
        return R.epi_none(P.y0), "eq"
    if epi in ALPHAS:
        return R.epi_scale(P.y0, ALPHAS[epi]), "eq"
    if epi in ("res", "res_inplace"):
        return R.epi_res(P.y, P.res), "eq"
    if epi in GATED:
        return R.epi_gate_res(P.y, P.res, P.gate, rows_per_batch), "eq"
    if epi in ACTIVATIONS:
        return (R.epi_gelu if epi == "gelu" else R.epi_silu)(P.act[1]), "ulp"
    raise ValueError(epi)


# ---- the data rules as predicates (asserted for every case by tests/test_gemm_large_host.py) ---------------------------------

def unit_sensitive(v):
    """bf16(v + 1) != bf16(v) and bf16(v - 1) != bf16(v) for every element of the fp64 tensor v."""
    b = v.to(F32).to(BF)
    return bool(((v + 1).to(F32).to(BF) != b).all() and ((v - 1).to(F32).to(BF) != b).all())


def rounding_points(epi, P, rows_per_batch=None):
    """The exact (fp64) values that a bf16-output equality case rounds to bf16: the staged y (+ bias), and what the residual
    forms store."""
    if epi in ("none", *ALPHAS):           # the scaled store has a predicate of its own: scale_is_sensitive
        return [P.y0]
    y = P.y
    if epi == "none_bias":
        return [y]
    res = P.res.to(F64)
    if epi in ("res", "res_inplace"):
        return [y, y + res]
    if epi in GATED:
        g = R.gate_rows(P.gate, rows_per_batch, P.M).to(F64)
        return [y, res + g * y]
    raise ValueError(epi)


def gate_is_exact(P, rows_per_batch):
    """Neither gate * bf16(y) nor its sum with the residual rounds, and the stored value moves when y moves by one."""
    y = P.y
    g = R.gate_rows(P.gate, rows_per_batch, P.M).to(F64)
    prod, total = g * y, P.res.to(F64) + g * y
    exact = lambda v: torch.equal(v.to(F32).to(BF).to(F64), v)      # noqa: E731
    stored = R.epi_gate_res(y, P.res, P.gate, rows_per_batch)
    return bool(exact(y) and exact(prod) and exact(total) and torch.equal(stored.to(F64), total)
                and (R.epi_gate_res(y + 1, P.res, P.gate, rows_per_batch) != stored).all()
                and (R.epi_gate_res(y - 1, P.res, P.gate, rows_per_batch) != stored).all())


def scale_is_sensitive(P, epi):
    """bf16(alpha * (y0 +- 1)) != bf16(alpha * y0) for every element: a unit in the sum survives the scaled store."""
    stored = R.epi_scale(P.y0, ALPHAS[epi])
    return bool((R.epi_scale(P.y0 + 1, ALPHAS[epi]) != stored).all() and (R.epi_scale(P.y0 - 1, ALPHAS[epi]) != stored).all())


def sample_rows(M, B, rows_per_batch):
    """Rows of a large problem on which the CPU checks its sums: the first row tile, the ragged last one, and the two rows at
    every batch boundary."""
    edges = torch.arange(1, B) * rows_per_batch
    return torch.cat([torch.arange(0, 256), torch.arange(M - M % 256, M), edges - 1, edges]).unique()


def big_bound_holds(P, epi):
    """For every element of a (tight) problem: |y| <= 255, and for the gated form 2 |y| + 16 <= 255, which keeps res + gate * y
    within 255 for every gate of {+-0.5, +-1, +-2} and every residual of [-16, 16] -- the unit sensitivity rule without forming
    the per-element values a second time."""
    top = P.y0.abs().max().item() + P.bias.float().abs().max().item()          # >= max |y|, without forming y
    return top <= 255 and (epi not in GATED or (2 * top + 16 <= 255 and P.res.float().abs().max().item() <= 16))


def gates_differ(P):
    """Neighbouring batches and neighbouring columns (and columns 8 / 128 / 256 apart) never share a gate value."""
    g = P.gate.float()
    ok = set(g.unique().tolist()) <= set(GATE_VALUES) and (g[:, 1:] != g[:, :-1]).all()
    for d in (8, 128, 256):
        ok = ok and (P.N <= d or (g[:, d:] != g[:, :-d]).all())
    return bool(ok and (P.B == 1 or (g[1:] != g[:-1]).all()))


# ---- every (data, epilogue) combination the GPU file builds --------------------------------------------------------------------

def host_cases(cus=256):
    """Sorted unique (section, M, N, K, B, R, epilogue) of everything tests/test_hip_gemm_large_exact.py launches (R = rows
    per batch of the gate, 0 without one; `cus` sizes section G).  The GPU file builds its problems through `case_problem`
    from the same tables, so what is asserted here is what runs there."""
    out = set()
    for form, shapes in A_SHAPES.items():
        out |= {("A", M, N, K, 1, 0, "f32") for M, N in shapes for K in A_KS}
    for form, shapes in B_SHAPES.items():
        out |= {("B", M, N, K, 1, M if epi in GATED else 0, epi) for M, N in shapes for K in B_KS for epi in EPILOGUES}
    out |= {("C", B * Rr, C_N, C_K, B, Rr if epi in GATED else 0, epi) for B, Rr in C_BR for epi in C_EPILOGUES}
    out |= {("D", B * Rr, D_N, D_K, B, Rr if epi in GATED else 0, epi) for B, Rr in D_BR for epi in D_EPILOGUES}
    out |= {("E", M, N, K, E_GATE_BR[0] if epi == "gate_res" else 1, E_GATE_BR[1] if epi == "gate_res" else 0, epi)
            for M, N in E_SHAPES for K in E_KS for epi in E_EPILOGUES if e_applies(M, N, K, epi)}
    out |= {("E", M, N, K, 1, 0, "none_bias") for M, N, K in E_SEQUENCE}
    out |= {("F", M, N, K, 2 if epi in GATED else 1, M // 2 if epi in GATED else 0, epi)
            for _, M, N, K in streamk_cases() for epi in F_EPILOGUES}
    M, N, B, Rr = persistent_grid(cus)
    out |= {("G", M, N, K, B, Rr, epi) for K in G_KS for epi in G_EPILOGUES}
    # W: what tests/test_hip_gemm_walk_exact.py builds (its part H runs section H's random data against the unfused launch)
    for part, form, Ms, N, K in walk_launches():
        if part == "A":
            out.add(("W", Ms[0], N, K, 1, 0, W_EPI_A))
        elif part == "B":
            out |= {("W", Ms[0], N, K, 1, Ms[0] if epi in GATED else 0, epi) for epi in EPILOGUES}
    out |= {("W", B * Rr, C_N, C_K, B, Rr if epi in GATED else 0, epi) for B, Rr in C_BR for epi in C_EPILOGUES}
    out |= {("W", B * Rr, D_N, D_K, B, Rr if epi in GATED else 0, epi) for B, Rr in D_BR for epi in D_EPILOGUES}
    out |= {("W", B * Rr, W_GM_N, W_GM_K, B, Rr if epi in GATED else 0, epi) for B, Rr in W_GM_BR for epi in D_EPILOGUES}
    return sorted(out)


def case_problem(M, N, K, B, epi, big=False):
    """The Problem of a case: tight data for the gated forms, the gate's batches only where there is a gate.  big (section
    G): one Problem (tight, with the gate's batches) serves all three epilogues of a K, so its product is formed once."""
    if big:
        return big_problem(M, N, K, B, True)
    return problem(M, N, K, B if epi in GATED else 1, epi in GATED)
