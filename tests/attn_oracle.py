"""An fp64 oracle of paged attention that works on absolute tokens, the cache builder that goes
with it, and the inputs (positional probes, peaked dense softmax) of test_attn_oracle_cpu.py and
test_attn_probes_gpu.py.

Nothing here calls ops/reference.py's slot arithmetic (_gather_seq, _ring_abs, _attend_one): the
oracle never looks at a cache.  It is given the tokens K_tok[a], V_tok[a] of a sequence, a = 0 ..,
and the rule of who sees whom:

    query at absolute position p sees token a  iff  a <= p  and, in window mode,
                                                    (a < n_sink or p - a < window - n_sink)

with tokens a < n_sink (window mode) scored against q_sink and all others against q.  The cache
builder is the other half: it writes the same tokens into paged caches the way a writer would
(token a to slot a, or to sink_pad + (a - n_sink) % ring once past the sinks, later tokens
overwriting earlier ones), so a kernel that gets a slot, a mask bit or a split wrong disagrees
with the oracle.

Tolerance (derived, see bound()): the kernels round P to bf16 before the PV product, sum l from
the unrounded p and round the output to bf16 once; everything else is fp32 on exact bf16
products (fp8 is widened exactly, V's scale is applied in fp32).  A bf16 rounding errs by 2^-9
relative on average over a binade and by 2^-8 (half an ulp of an 8-bit significand) at worst, so
per element the P rounding gives about 2^-9 * A (A = sum_j p_j |v_j|) and the output rounding
2^-9 * |o|.  The tests accept twice that, 2^-8 * (A + |o|) + 1e-6: it covers both roundings at
their worst plus, in all but that corner, exp2, fp32 accumulation order and the split merges.
Measured on an MI355X the kernels use up to 0.73 of it on the probes of decode, 0.88 on those
of prefill, and up to 0.94 on peaked dense prefill data (where one output element is a single
p * v product and both roundings can be near their worst at once).
"""
import dataclasses
import functools
import math
from typing import List, Optional, Tuple

import numpy as np
import torch

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
POISON = 240.0          # finite stale-slot fill: representable in bf16 and e4m3


# ------------------------------------------------------------------------------------ geometry
@dataclasses.dataclass(frozen=True)
class Geo:
    nh: int
    nkv: int
    D: int
    fp8: bool = False
    n_sink: int = 0
    sink_pad: int = 0
    ring: int = 0
    window: int = 0
    bs: int = 64

    @property
    def k_scale(self):
        return 0.25 if self.fp8 else 1.0

    @property
    def v_scale(self):
        return 1.5 if self.fp8 else 1.0

    @property
    def scale(self):
        return 1.0 / math.sqrt(self.D)

    @property
    def win(self):
        return self.ring > 0

    @property
    def G(self):
        return self.nh // self.nkv

    def window_args(self):
        return (self.n_sink, self.sink_pad, self.ring, self.window)


def slot_of(a, g: Geo):
    """The writer's rule: the cache slot of absolute token(s) ``a`` (numpy array or int)."""
    a = np.asarray(a)
    if not g.win:
        return a
    return np.where(a < g.n_sink, a, g.sink_pad + (a - g.n_sink) % g.ring)


def _stored(x: torch.Tensor, scale: float, fp8: bool) -> torch.Tensor:
    """What the cache holds for token values x: bf16, or e4m3 of x / scale."""
    x = x.to(BF)
    return (x.float() / scale).to(F8) if fp8 else x


def rounded(x: torch.Tensor, scale: float, fp8: bool) -> torch.Tensor:
    """Token values as the kernels see them (cache-rounded, dequantised), fp64."""
    return _stored(x, scale, fp8).double() * (scale if fp8 else 1.0)


def _filled(shape, poison: bool, dtype, seed: int) -> torch.Tensor:
    if not poison:
        return torch.zeros(shape, dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    pat = (torch.randint(0, 2, shape[-3:], generator=g).float() * 2 - 1) * POISON
    return pat.expand(shape).contiguous().to(dtype)


def build_caches(g: Geo, K_tok: List[torch.Tensor], V_tok: List[torch.Tensor], seq_lens,
                 q_lens=None, poison: bool = False, seed: int = 0):
    """Paged caches holding the tokens ``K_tok[b] / V_tok[b]`` ([n_written, nkv, D] each; a
    sequence may hold tokens past its ``seq_lens[b]``: stale slots with real data in them).
    Every slot not written holds the fill (0, or +-POISON): the rest of a page, the gap
    [n_sink, sink_pad), ring slots not reached, two pages outside every table and one spare page
    that all unused block-table columns name.  K is [blocks, nkv, bs, D], V is V^T in 8-key groups
    [blocks, nkv, bs/8, D, 8]; the block tables are a random permutation.
    Returns (k_cache, v_cache, block_tables int32 [B, max_blocks])."""
    B, bs = len(K_tok), g.bs
    pages = []
    for b in range(B):
        nw, L = K_tok[b].shape[0], int(seq_lens[b])
        assert nw >= L and V_tok[b].shape == K_tok[b].shape
        if g.win:
            ql = int(q_lens[b]) if q_lens is not None else 1
            # the block manager's sizing: no token a query may see has been overwritten
            assert g.ring >= g.window - g.n_sink + ql - 1 + (nw - L), (g, ql, nw, L)
            assert g.sink_pad >= g.n_sink and g.window > g.n_sink
            pages.append((g.sink_pad + g.ring + bs - 1) // bs)
        else:
            pages.append((nw + bs - 1) // bs)
    max_blocks = max(1, max(pages))
    nblocks = sum(pages) + 3
    perm = torch.randperm(nblocks, generator=torch.Generator().manual_seed(seed)).tolist()
    spare, free = perm[0], perm[3:]          # perm[1], perm[2]: pages outside every table
    bt = torch.full((B, max_blocks), spare, dtype=torch.int32)
    cdt = F8 if g.fp8 else BF
    kc = _filled((nblocks, g.nkv, bs, g.D), poison, cdt, seed + 1)
    vc = _filled((nblocks, g.nkv, bs // 8, g.D, 8), poison, cdt, seed + 2)
    for b in range(B):
        mine, free = free[:pages[b]], free[pages[b]:]
        bt[b, :pages[b]] = torch.tensor(mine, dtype=torch.int32)
        nw = K_tok[b].shape[0]
        if nw == 0:
            continue
        a = np.arange(nw)
        owner = np.full(pages[b] * bs, -1, dtype=np.int64)
        owner[slot_of(a, g)] = a             # written in order: the last token of a slot stays
        slots = np.nonzero(owner >= 0)[0]
        tok = torch.from_numpy(owner[slots])
        s = torch.from_numpy(slots)
        page, off = bt[b, s // bs].long(), s % bs
        kc[page, :, off, :] = _stored(K_tok[b][tok], g.k_scale, g.fp8)
        vc[page, :, off // 8, :, off % 8] = _stored(V_tok[b][tok], g.v_scale, g.fp8)
    return kc, vc, bt


# ------------------------------------------------------------------------------------- oracle
def visible(qpos: torch.Tensor, n_tok: int, g: Geo) -> torch.Tensor:
    """[n, n_tok] bool: which tokens each query position sees."""
    a = torch.arange(n_tok)
    vis = a[None, :] <= qpos[:, None]
    if g.win:
        vis &= (a < g.n_sink)[None, :] | ((qpos[:, None] - a[None, :]) < (g.window - g.n_sink))
    return vis


def attend(q, q_sink, qpos, Kr, Vr, g: Geo, vis=None, sinks_with_q=False):
    """fp64 attention of queries q [n, nh, D] at absolute positions qpos [n] over the tokens
    Kr / Vr [n_tok, nkv, D] (fp64, cache-rounded).  Returns (o, A, P): the output, the
    absolute-weighted sum A = sum_j p_j |v_j| (both [n, nh, D]) and the weights [n, nh, n_tok].
    A row with no visible key gives zeros.  ``vis`` overrides the visibility (mutations)."""
    n, S = q.shape[0], Kr.shape[0]
    if vis is None:
        vis = visible(qpos, S, g)
    qg = q.double().reshape(n, g.nkv, g.G, g.D)
    s = torch.einsum("nkgd,skd->nkgs", qg, Kr) * g.scale
    if g.win and g.n_sink > 0 and not sinks_with_q:
        ns = min(g.n_sink, S)
        qs = q_sink.double().reshape(n, g.nkv, g.G, g.D)
        s[..., :ns] = torch.einsum("nkgd,skd->nkgs", qs, Kr[:ns]) * g.scale
    s = s.masked_fill(~vis[:, None, None, :], float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    P = torch.where(l > 0, e / l, torch.zeros_like(e))
    o = torch.einsum("nkgs,skd->nkgd", P, Vr).reshape(n, g.nh, g.D)
    A = torch.einsum("nkgs,skd->nkgd", P, Vr.abs()).reshape(n, g.nh, g.D)
    return o, A, P.reshape(n, g.nh, S)


def bound(o: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """2 * (2^-9 A + 2^-9 |o|) + 1e-6: see the module docstring."""
    return 2.0 ** -8 * (A + o.abs()) + 1e-6


# -------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Spec:
    """One set of inputs.  ``lens``: decode: the sequence lengths (each repeated over as many
    rows as its probe targets need); prefill: unused.  ``q_lens`` / ``ctx``: prefill chunks.
    ``data``: 'probe', 'asc' or 'desc' (peaked dense softmax, keys sorted by the score of head
    0 ascending / descending along the sequence)."""
    kind: str                       # 'decode' | 'prefill'
    geo: Geo
    lens: Tuple[int, ...] = ()
    q_lens: Tuple[int, ...] = ()
    ctx: Tuple[int, ...] = ()
    data: str = "probe"
    seed: int = 0
    rows: int = 0                   # decode: > 0: exactly this many rows, lens cycled

    def ident(self):
        g = self.geo
        w = f"-w{g.window}s{g.n_sink}r{g.ring}" if g.win else ""
        return (f"{self.kind}-{g.nh}x{g.nkv}x{g.D}-{'fp8' if g.fp8 else 'bf16'}{w}-{self.data}"
                + (f"-B{self.rows}" if self.rows else ""))


@dataclasses.dataclass
class Case:
    spec: Spec
    seq_lens: List[int]             # per sequence
    q_lens: List[int]               # per sequence (1 for decode; 0 for an empty decode row)
    K_tok: List[torch.Tensor]       # per sequence [n_written, nkv, D] fp32
    V_tok: List[torch.Tensor]
    q: torch.Tensor                 # [T, nh, D] bf16
    q_sink: Optional[torch.Tensor]
    seq_of: torch.Tensor            # [T] sequence of each query row
    qpos: torch.Tensor              # [T] absolute position of each query row
    target: torch.Tensor            # [T, nh] the token a probe must return (-1: none dominates)
    tq: torch.Tensor                # [T, nh] token whose code is in q (-1: zeros)
    ts: torch.Tensor                # [T, nh] token whose code is in q_sink (-1: zeros)

    @property
    def geo(self):
        return self.spec.geo

    def q_start(self):
        return torch.tensor([0] + list(np.cumsum(self.q_lens)), dtype=torch.int32)

    def rows_of(self, b):
        return (self.seq_of == b).nonzero().flatten()

    def Kr(self, b):
        return rounded(self.K_tok[b], self.geo.k_scale, self.geo.fp8)

    def Vr(self, b):
        return rounded(self.V_tok[b], self.geo.v_scale, self.geo.fp8)

    def caches(self, poison: bool):
        return build_caches(self.geo, self.K_tok, self.V_tok, self.seq_lens,
                            self.q_lens if self.spec.kind == "prefill" else None, poison,
                            seed=self.spec.seed + 100)


BETA = {128: 4.0, 64: 8.0, 32: 16.0}    # probe strength: q = BETA * code (exact in bf16)


def _codes(n, nkv, D, gen):
    """Sign codes [n, nkv, D] in {+1, -1}: exact in bf16 and (divided by 0.25) in e4m3."""
    return torch.randint(0, 2, (n, nkv, D), generator=gen).float() * 2 - 1


def _values(n, nkv, D, gen, v_scale):
    """V rows on the e4m3-exact grid {k/4 : |k| <= 15} (times the cache's scale, so that the
    stored value is on the grid), distinct per token."""
    v = torch.randint(-15, 16, (n, nkv, D), generator=gen).float() / 4
    flat = v.permute(1, 0, 2)
    for h in range(nkv):
        assert torch.unique(flat[h], dim=0).shape[0] == n, "V rows must be distinct"
    return v * v_scale


def _multiples_both_sides(lo, hi, step, phase=0):
    """Tokens on both sides of every boundary a with (a - phase) % step == 0, lo < a <= hi."""
    out = []
    for a in range(lo + 1, hi + 1):
        if (a - phase) % step == 0:
            out += [a - 1, a]
    return out


def decode_targets(L: int, g: Geo):
    """(tq, ts) pairs of one decode length: the token whose code goes into q and the one that
    goes into q_sink (-1: zeros).  The sequence holds L + 1 tokens: token L is stale."""
    p = L - 1
    if not g.win:
        if L == 0:
            return [(0, -1)]
        t = [0, L - 1] + _multiples_both_sides(0, L - 1, 8) + [L]     # L: stale, same page
        return [(a, -1) for a in dict.fromkeys(t)]
    ns, W = g.n_sink, g.window - g.n_sink
    out = []
    lo = max(ns, p - W + 1)                  # oldest visible rolling token
    roll = [L - 1, lo] + _multiples_both_sides(lo, L - 1, 8, phase=ns) if L > ns else []
    roll = list(dict.fromkeys(roll))
    sink_decoy = (lambda a: (a + 1) % ns) if ns > 1 else (lambda a: -1)
    for i, a in enumerate(roll):
        other = roll[(i + 1) % len(roll)] if len(roll) > 1 else -1
        out.append((a, other))               # q_sink carries another rolling token's code
    if L > ns and lo - 1 >= ns:
        out.append((lo - 1, lo))             # invisible: just left the window, still in the ring
    out.append((L, L - 1 if L - 1 >= ns else -1))    # invisible: stale token past the end
    for s in range(min(ns, L)):
        out.append((sink_decoy(s) if min(ns, L) > 1 else L, s))      # sink through q_sink
        out.append((s, L - 1 if L - 1 >= ns else -1))   # invisible: sink code in q
    return out


def prefill_targets(t: int, h: int, ctx: int, g: Geo):
    """(tq, ts) of head h of the chunk's query token t (absolute position p = ctx + t)."""
    p, j = ctx + t, h // 5
    ns = g.n_sink if g.win else 0

    def via(a):   # a token meant to be seen: through q, or through q_sink if it is a sink
        if a < ns:
            return ((a + 1) % ns if ns > 1 else -1, a)
        return (a, a + 1)     # q_sink carries a rolling token's code (never scored with it)

    if not g.win:
        k = (t + h) % 5
        if k == 0:
            return via(max(0, p - 2 * j))            # the diagonal (j = 0) and near it
        if k == 1:
            return via(max(0, p - 1 - 2 * j))
        if k == 2:
            return via(min(j, p))                    # key 0
        if k == 3:
            return via(min(ctx + j, p))              # first key of the chunk
        return (p + 1, -1)                           # invisible: the next key of the chunk
    W = g.window - ns
    lo = max(ns, p - W + 1) if p >= ns else p + 1    # oldest visible rolling token
    k = (t + h) % 8
    if k == 0:
        return via(p)
    if k == 1:
        return via(max(p - 1, min(lo, p)))
    if k == 2:
        return via(min(lo + j, p))
    if k == 3:
        return via(min(max(ctx, lo) + j, p))
    if k == 4:
        return (p + 1, p + 1)
    if k == 5:
        return (lo - 1, p) if lo - 1 >= ns and lo <= p else (p + 1, p + 1)   # just expired
    if ns == 0:
        return via(max(lo, p - 3 - j)) if k == 6 else (0, -1)    # key 0: seen only if p < window
    s = h % min(ns, p + 1)
    if k == 6:
        return via(s)                                # a sink through q_sink
    return (s, p if p >= ns else p + 1)              # invisible: sink code in q


def _dominant(tq, ts, p, g: Geo):
    """The token a probe's weight must sit on, by the visibility rule (-1: none)."""
    ns = g.n_sink if g.win else 0
    dom = -1
    if ns <= tq <= p and (not g.win or p - tq < g.window - ns):
        dom = tq
    if 0 <= ts < ns and ts <= p:
        assert dom < 0, "a probe must not point q and q_sink at two visible tokens"
        dom = ts
    return dom


@functools.lru_cache(maxsize=8)
def make_case(spec: Spec) -> Case:
    g = spec.geo
    gen = torch.Generator().manual_seed(1000 + spec.seed)
    seq_lens, q_lens, ctxs, plans = [], [], [], []
    if spec.kind == "decode":
        if spec.rows:
            lens = [spec.lens[i % len(spec.lens)] for i in range(spec.rows)]
            plan_of = {L: decode_targets(L, g) for L in spec.lens}
            seen = {L: 0 for L in spec.lens}
            for L in lens:       # every row of a length continues that length's target list
                tg = plan_of[L]
                plans.append([[tg[(seen[L] + h) % len(tg)] for h in range(g.nh)]])
                seen[L] += g.nh
                seq_lens.append(L)
        elif spec.data != "probe":
            seq_lens = list(spec.lens)
            plans = [None] * len(seq_lens)
        else:
            for L in spec.lens:
                tg = decode_targets(L, g)
                for r in range((len(tg) + g.nh - 1) // g.nh):
                    plans.append([[tg[(r * g.nh + h) % len(tg)] for h in range(g.nh)]])
                    seq_lens.append(L)
        q_lens = [1] * len(seq_lens)
        ctxs = [max(L - 1, 0) for L in seq_lens]
    else:
        for ql, c in zip(spec.q_lens, spec.ctx):
            plans.append([[prefill_targets(t, h, c, g) for h in range(g.nh)] for t in range(ql)])
            seq_lens.append(ql + c)
            q_lens.append(ql)
            ctxs.append(c)
    B, T = len(seq_lens), sum(q_lens)
    K_tok, V_tok = [], []
    for b in range(B):
        nw = seq_lens[b] + 1                 # one stale token past the end
        if spec.data == "probe":
            K_tok.append(_codes(nw, g.nkv, g.D, gen))
            V_tok.append(_values(nw, g.nkv, g.D, gen, g.v_scale))
        else:
            K_tok.append(torch.randn(nw, g.nkv, g.D, generator=gen))
            V_tok.append(torch.randn(nw, g.nkv, g.D, generator=gen))
    q = torch.zeros(T, g.nh, g.D)
    qs = torch.zeros(T, g.nh, g.D)
    seq_of = torch.zeros(T, dtype=torch.long)
    qpos = torch.zeros(T, dtype=torch.long)
    target = torch.full((T, g.nh), -1, dtype=torch.long)
    tq_all = torch.full((T, g.nh), -1, dtype=torch.long)
    ts_all = torch.full((T, g.nh), -1, dtype=torch.long)
    row = 0
    for b in range(B):
        for t in range(q_lens[b]):
            seq_of[row], qpos[row] = b, ctxs[b] + t
            if spec.data == "probe":
                kvh = torch.arange(g.nh) // g.G
                pl = plans[b][t]
                tq = torch.tensor([min(a, seq_lens[b]) for a, _ in pl])
                ts = torch.tensor([min(a, seq_lens[b]) for _, a in pl])
                q[row] = torch.where((tq >= 0)[:, None],
                                     K_tok[b][tq.clamp(min=0), kvh] * BETA[g.D], q[row])
                qs[row] = torch.where((ts >= 0)[:, None],
                                      K_tok[b][ts.clamp(min=0), kvh] * BETA[g.D], qs[row])
                tq_all[row], ts_all[row] = tq, ts
                if seq_lens[b] > 0:
                    for h in range(g.nh):
                        target[row, h] = _dominant(int(tq[h]), int(ts[h]), int(qpos[row]), g)
            row += 1
    if spec.data != "probe":
        # natural-log logits of std 5: a handful of keys carry the weight, the running max moves
        q = torch.randn(T, g.nh, g.D, generator=gen) * 5.0
        qs = torch.randn(T, g.nh, g.D, generator=gen) * 5.0
        for b in range(B):
            rows = (seq_of == b).nonzero().flatten()
            qlast = q[rows[-1], 0].to(BF).double()
            sc = rounded(K_tok[b], g.k_scale, g.fp8)[:, 0] @ qlast
            order = torch.argsort(sc, descending=(spec.data == "desc"))
            K_tok[b], V_tok[b] = K_tok[b][order], V_tok[b][order]
    use_sink = g.win and g.n_sink > 0
    return Case(spec, seq_lens, q_lens, K_tok, V_tok, q.to(BF), qs.to(BF) if use_sink else None,
                seq_of, qpos, target, tq_all, ts_all)


def case_visible(c: Case, b: int, rows: torch.Tensor) -> torch.Tensor:
    """Visibility of sequence b's tokens (stale one included) to its query rows."""
    vis = visible(c.qpos[rows], c.K_tok[b].shape[0], c.geo)
    if c.seq_lens[b] == 0:
        vis[:] = False
    return vis


@functools.lru_cache(maxsize=8)
def oracle(spec: Spec, sample: Optional[Tuple[int, ...]] = None):
    """(o, A, P-weight of every probe's target) of a case: o, A [T, nh, D] fp64; rows of
    sequences outside ``sample`` (a tuple of sequence indices) are left NaN."""
    c = make_case(spec)
    g = c.geo
    T = c.q.shape[0]
    o = torch.full((T, g.nh, g.D), float("nan"), dtype=torch.float64)
    A = torch.full_like(o, float("nan"))
    wt = torch.full((T, g.nh), float("nan"), dtype=torch.float64)
    for b in (range(len(c.seq_lens)) if sample is None else sample):
        rows = c.rows_of(b)
        if rows.numel() == 0:
            continue
        ob, Ab, P = attend(c.q[rows], c.q_sink[rows] if c.q_sink is not None else None,
                           c.qpos[rows], c.Kr(b), c.Vr(b), g, vis=case_visible(c, b, rows))
        o[rows], A[rows] = ob, Ab
        tg = c.target[rows]
        wt[rows] = torch.where(tg >= 0, P.gather(2, tg.clamp(min=0)[..., None])[..., 0],
                               torch.full_like(tg, float("nan"), dtype=torch.float64))
    return o, A, wt


def mutated(spec: Spec, kind: str, splits: int = 1, split: int = 0):
    """The oracle's output under one deliberate mistake (teeth checks).  Returns (o_mut, hit):
    hit[T] says which query rows the mutation changed the visibility or scoring of."""
    c = make_case(spec)
    g = c.geo
    ns = g.n_sink if g.win else 0
    T = c.q.shape[0]
    o = torch.zeros(T, g.nh, g.D, dtype=torch.float64)
    hit = torch.zeros(T, dtype=torch.bool)
    for b in range(len(c.seq_lens)):
        rows = c.rows_of(b)
        if rows.numel() == 0:
            continue
        Kr, Vr = c.Kr(b), c.Vr(b)
        S = Kr.shape[0]
        qp = c.qpos[rows]
        vis0 = case_visible(c, b, rows)
        vis = vis0.clone()
        a = torch.arange(S)
        n = torch.arange(rows.numel())
        roll = vis0 & (a >= ns)[None, :]
        if kind == "drop_newest":
            vis[n, qp.clamp(max=S - 1)] = False
        elif kind == "drop_oldest":
            first = vis0.float().argmax(1)
            vis[n, first] = False
        elif kind == "drop_oldest_rolling":
            first = roll.float().argmax(1)
            vis[n, first] &= ~roll.any(1)
        elif kind == "admit_next":
            vis[n, (qp + 1).clamp(max=S - 1)] = True
        elif kind == "admit_expired":
            first = roll.float().argmax(1)
            ok = roll.any(1) & (first - 1 >= ns)
            vis[n[ok], first[ok] - 1] = True
        elif kind == "drop_split":
            # the keys of one split's 32-slot steps (rolling / full segment, in slot order)
            L = c.seq_lens[b]
            seg = (min(g.ring, L - ns) if L > ns else 0) if g.win else L
            nsteps = (seg + 31) // 32
            per = (nsteps + splits - 1) // splits
            off = torch.from_numpy(np.asarray(slot_of(a.numpy(), g))) - (g.sink_pad if g.win else 0)
            in_split = (a >= ns) & (off // 32 >= split * per) & (off // 32 < (split + 1) * per)
            vis &= ~in_split[None, :]
        elif kind != "sinks_with_q":
            raise ValueError(kind)
        if c.seq_lens[b] == 0:
            vis[:] = False
        swq = kind == "sinks_with_q"
        hit[rows] = (vis != vis0).any(1) | (swq and ns > 0)
        o[rows] = attend(c.q[rows], c.q_sink[rows] if c.q_sink is not None else None, qp, Kr, Vr,
                         g, vis=vis, sinks_with_q=swq)[0]
    return o, hit


def nearest_v_row(c: Case, row: int, head: int, out_row: torch.Tensor) -> int:
    """Which token's V row an output row is closest to (failure messages)."""
    b = int(c.seq_of[row])
    V = c.Vr(b)[:, head // c.geo.G]
    return int((V - out_row.double()[None, :]).abs().amax(1).argmin())


# -------------------------------------------------------------------------- the case matrix
DECODE_LENS = (0, 1, 31, 32, 33, 63, 64, 65, 97, 128, 129, 257)
DECODE_SPLITS = (1, 2, 3, 4, 6, 12)
WINDOW_LENS = (1, 3, 4, 5, 36, 99, 100, 101, 131, 132, 133, 260, 517)
WINDOW_SPLITS = (1, 2, 4)
ONE_STEP_LENS = (1, 31, 32, 33, 64, 65, 100)
PREFILL_Q = (1, 15, 16, 17, 33, 65, 130)
PREFILL_CTX = (129, 0, 10, 63, 64, 70, 0)


def _ceil32(x):
    return (x + 31) // 32 * 32


def decode_full_specs():
    out = []
    for D in (32, 64, 128):
        for fp8 in (False, True):
            # D = 32: random sign codes are thin at 257 keys, BETA = 16 makes up for it (the
            # weight assert of test_attn_oracle_cpu.py holds with 10^-10 to spare)
            out.append(Spec("decode", Geo(8, 2, D, fp8), lens=DECODE_LENS, seed=D + fp8))
    return out


def decode_head_specs():
    return [Spec("decode", Geo(nh, nkv, 128, fp8), lens=DECODE_LENS, seed=nh + fp8)
            for nh, nkv in ((8, 8), (28, 4), (32, 2), (40, 2), (64, 2)) for fp8 in (False, True)]


def decode_one_step_specs():
    return [Spec("decode", Geo(8, 8, 128, fp8), lens=ONE_STEP_LENS, rows=512, seed=7 + fp8)
            for fp8 in (False, True)]


def _wgeo(nh, nkv, D, fp8, n_sink=4):
    return Geo(nh, nkv, D, fp8, n_sink=n_sink, sink_pad=32 if n_sink else 0, ring=128, window=100)


def decode_window_specs():
    out = [Spec("decode", _wgeo(8, 2, 128, fp8), lens=WINDOW_LENS, seed=20 + fp8)
           for fp8 in (False, True)]
    out.append(Spec("decode", _wgeo(8, 2, 64, False), lens=WINDOW_LENS, seed=22))
    out.append(Spec("decode", _wgeo(8, 2, 128, False, n_sink=0), lens=WINDOW_LENS, seed=23))
    # two 16-head groups, the second with 4 live columns, through the sink step
    out.append(Spec("decode", _wgeo(40, 2, 128, True), lens=WINDOW_LENS, seed=24))
    return out


def _pgeo(nh, nkv, D, fp8=False, n_sink=0, window=0):
    if not window:
        return Geo(nh, nkv, D, fp8)
    sink_pad = _ceil32(n_sink)
    # the block manager's rule, with room for the one stale token past the end
    ring = _ceil32(window - n_sink + max(PREFILL_Q))
    return Geo(nh, nkv, D, fp8, n_sink=n_sink, sink_pad=sink_pad, ring=ring, window=window)


def _pspec(geo, seed, data="probe"):
    q_lens, ctx = PREFILL_Q, PREFILL_CTX
    if geo.win:
        # one chunk on top of a ring that has wrapped: with the lengths above alone no token
        # would ever leave a 200-token window
        q_lens, ctx = q_lens + (40,), ctx + (700,)
    return Spec("prefill", geo, q_lens=q_lens, ctx=ctx, data=data, seed=seed)


def prefill_legacy_specs():
    """attention.hip's prefill kernel: (spec, [(qb, tile map)])."""
    every = [(1, False), (1, True), (2, False), (2, True)]
    out = [(_pspec(_pgeo(nh, nkv, 128), 30 + nh), every) for nh, nkv in ((8, 2), (6, 3), (7, 7))]
    out += [(_pspec(_pgeo(8, 2, D), 40 + D), every) for D in (32, 64)]
    out.append((_pspec(_pgeo(8, 2, 128, fp8=True), 45), [(1, True), (2, False)]))
    out += [(_pspec(_pgeo(8, 2, 128, n_sink=ns, window=96), 46 + ns), [(1, True), (2, False)])
            for ns in (0, 4)]
    out.append((_pspec(_pgeo(6, 3, 64, n_sink=4, window=96), 52), [(1, False), (2, True)]))
    return out


def prefill_m32_specs():
    """attn_prefill32.hip: (spec, [qb]) with only the combinations the kernel is eligible for
    (groups that are no multiple of 4 need qb = 2; fp8: groups of 8, or qb = 2)."""
    out = []
    for nh, nkv in ((64, 8), (16, 4), (16, 8), (16, 16)):
        G = nh // nkv
        qbs = [1, 2] if G % 4 == 0 else [2]
        out.append((_pspec(_pgeo(nh, nkv, 128), 60 + nh + nkv), qbs))
        out.append((_pspec(_pgeo(nh, nkv, 128, fp8=True), 61 + nh + nkv),
                    [1, 2] if G % 8 == 0 else [2]))
    for ns in (0, 4, 40):
        out.append((_pspec(_pgeo(16, 4, 128, n_sink=ns, window=200), 90 + ns), [1, 2]))
    out.append((_pspec(_pgeo(16, 16, 128, n_sink=4, window=200), 95), [2]))
    out.append((_pspec(_pgeo(64, 8, 128, fp8=True, n_sink=4, window=200), 96), [1, 2]))
    return out


DENSE_LENS = (33, 129, 257, 517)


def dense_specs():
    """Peaked dense softmax, both orderings, one representative shape per kernel family:
    (family, spec)."""
    out = []
    for data in ("asc", "desc"):
        for fp8 in (False, True):
            fam = "decode-fp8" if fp8 else "decode-bf16"
            out.append((fam, Spec("decode", Geo(16, 2, 128, fp8), lens=DENSE_LENS, data=data,
                                  seed=110 + fp8)))
            out.append(("decode-window", Spec("decode", _wgeo(16, 2, 128, fp8), lens=DENSE_LENS,
                                              data=data, seed=112 + fp8)))
        out.append(("prefill-legacy", _pspec(_pgeo(8, 2, 128), 120, data)))
        out.append(("prefill-legacy-window", _pspec(_pgeo(8, 2, 128, n_sink=4, window=96), 121,
                                                    data)))
        out.append(("prefill-m32", _pspec(_pgeo(16, 4, 128), 122, data)))
        out.append(("prefill-m32-window", _pspec(_pgeo(16, 4, 128, n_sink=4, window=200), 123,
                                                 data)))
    return out
