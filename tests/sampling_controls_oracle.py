"""CPU oracle of the sampling controls: the penalty kernels (csrc/kernels/penalty.hip) and the
sampler's min-p predicate (csrc/kernels/sampling.hip), on top of ``sampling_oracle``.

Penalties (vLLM / HF semantics), per row, before the temperature.  ``ctx`` = the prompt's token
set, ``n_out[t]`` = times ``t`` was generated, ``seen = ctx | (n_out > 0)``::

    v = l                      unseen tokens: untouched, bit for bit
    v = l / r if l > 0 else l * r          (seen)
    v = v - f * n_out                      (generated tokens only: n_out = 0 elsewhere)
    v = v - p * [n_out > 0]

evaluated in float64 from the fp32 values of r, f, p the kernel reads.  The expected bf16 logit
is the RNE rounding of ``v``.

Error bound of the kernel's fp32 evaluation (u = 2^-24, the unit roundoff of fp32).  The kernel
does three operations, each rounded once: a1 = fl(l / r) or fl(l * r); a2 = fma(-f, n, a1) (n is
exact in fp32); a3 = fl(a2 - p).  With M = max(|l|, |a1|, |f n|, |p|): |a1| <= M, |a2| <= 2M,
|a3| <= 3M, and each rounding adds at most u times the magnitude of its result, so the kernel's
value is within (1 + 2 + 3) u M = 6 u M of ``v`` (second-order terms are below u^2 M).  The
oracle itself rounds ``v`` to bf16 through fp32 (torch has no direct float64 -> bf16 cast), which
can move it by another u |v| <= 3 u M before the bf16 rounding.  ``E = 12 u M`` covers both with
room to spare: an element is *ambiguous* when bf16(v - E) != bf16(v + E), i.e. ``v`` lies within E
of a bf16 rounding midpoint, and then either neighbour is accepted.  A row without ambiguous
elements is *exact*.  fp32 logits are compared within the same E.  Non-finite values (a -inf
logit stays -inf under every operation) compare exactly.

An operation whose exact result is an fp32 number is not rounded at all.  bf16 logits have 8
significant bits, so this is the common case (l * 1.5, l - 2, l - 0.5 n ...), and such results
often fall *exactly* on a bf16 midpoint, where RNE - not an error - decides.  So E = 0 for an
element whose three intermediate values (evaluated in float64, where these few-bit products, sums
and exact quotients are exact) are all fp32 numbers: the kernel's value then equals ``v`` and
its bf16 rounding is determined, ties included.

min-p: with ``x = l / T`` over the penalised row (float64, as in ``sampling_oracle.scaled``) the
kernel keeps ``fl(l * fl(1/T)) >= fl(mx + logf(m))``, the fp32 form of ``x - mx >= ln m``.
fl(1/T) and the product each carry a relative error u, so the kernel's x (and its maximum mx, the
same formula on the largest element) are within 2u|x| (2u|mx|) of the float64 values; logf is
taken as accurate to 2 ulp = 4u|ln m|; the sum mx + ln m is rounded once, u|mx + ln m| <=
u(|mx| + |ln m|).  In all the fp32 bound of ``x - mx - ln m`` is 2u|x| + 3u|mx| + 5u|ln m|; the
oracle uses ``delta = 6u(|x| + |mx| + |ln m|)`` per element::

    must_keep &= (x >= mx + ln m + delta) | (x == mx)
    may_keep  &= (x >= mx + ln m - delta)

The maximum element compares exactly (the kernel's product for it *is* its mx), so m = 1 keeps the
maximum value group.  m = 0 is off; greedy rows ignore min-p.  Decisive rows as in ``RowOracle``.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

import sampling_oracle as so

U32 = 2.0 ** -24
PROMPT_BIT = -(1 << 31)
VOCABS = (8, 1003, 32776, 128256)   # scalar path, odd V, the NV 4 -> 8 edge, Llama-3
SLOTS = 8
MAX_AMBIGUOUS = 0.01                # of the touched elements (a condition, not a fit)
MIN_EXACT_DECISIVE = 0.90           # of the rows of the whole case set (a condition, not a fit)


def _bf16(x64: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.asarray(x64, dtype=np.float64)).to(torch.float32).to(torch.bfloat16)


def _is_f32(x64: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return x64.astype(np.float32).astype(np.float64) == x64


def f32(v) -> float:
    return float(np.float32(v))


# ------------------------------------------------------------------ penalties
@dataclass
class PenaltyOracle:
    value: np.ndarray          # float64 penalised row
    bound: np.ndarray          # E per element (0 where untouched)
    touched: np.ndarray        # bool: seen tokens (the kernel stores exactly these)
    expect: torch.Tensor       # bf16 RNE of value
    lo: torch.Tensor           # bf16(value - E), bf16(value + E): the accepted neighbours
    hi: torch.Tensor
    ambiguous: np.ndarray      # bool

    @property
    def exact(self) -> bool:
        return not bool(self.ambiguous.any())


def penalise_row(logits_row, in_prompt: np.ndarray, n_out: np.ndarray, r: float, f: float,
                 p: float) -> PenaltyOracle:
    l = np.asarray(logits_row, dtype=np.float64)
    r, f, p = f32(r), f32(f), f32(p)
    n = np.asarray(n_out, dtype=np.float64)
    gen = n > 0
    seen = np.asarray(in_prompt, dtype=bool) | gen
    with np.errstate(invalid="ignore", over="ignore"):
        a1 = np.where(l > 0, l / r, l * r)
        a2 = np.where(gen, a1 - f * n, a1)
        a3 = np.where(gen, a2 - p, a2)
        v = np.where(seen, a3, l)
        M = np.maximum.reduce([np.abs(l), np.abs(a1), np.abs(f * n), np.full_like(l, abs(p))])
        rounded = ~(_is_f32(a1) & _is_f32(a2) & _is_f32(a3))
        E = np.where(seen & np.isfinite(v) & rounded, 12.0 * U32 * M, 0.0)
        lo, hi = _bf16(v - E), _bf16(v + E)
    amb = (lo.view(torch.int16) != hi.view(torch.int16)).numpy() & seen
    return PenaltyOracle(v, E, seen, _bf16(v), lo, hi, amb)


def table_row(V: int, prompt: List[int], outputs: List[int]) -> np.ndarray:
    """The int32 table words of a sequence: bit 31 = in the prompt, bits 0-30 = n_out."""
    w = np.zeros(V, dtype=np.int64)
    for t, c in zip(*np.unique(np.asarray(outputs, dtype=np.int64), return_counts=True)):
        w[t] = c
    w[np.unique(np.asarray(prompt, dtype=np.int64))] += PROMPT_BIT
    return w.astype(np.int32)


# ------------------------------------------------------------------ min-p
def sample_row(logits_row, temperature: float, top_k: int = 0, top_p: float = 1.0,
               min_p: float = 0.0, seed: int = so.DEFAULT_SEED, row: int = 0,
               counter: Optional[int] = None, step: int = 0) -> so.RowOracle:
    """``sampling_oracle.sample_row`` with the min-p predicate on the kept sets."""
    m = f32(min_p)
    if not temperature > 0 or not m > 0:
        return so.sample_row(logits_row, temperature, top_k, top_p, seed, row, counter, step)
    lg = np.asarray(logits_row, dtype=np.float64)
    V = lg.shape[0]
    x = so.scaled(lg, temperature)
    must, may = so.kept_sets(x, int(top_k), float(top_p))
    finite = x > -np.inf
    if finite.any():
        must, may = must & finite, may & finite
    mx, ln_m = x.max(), math.log(m)
    with np.errstate(invalid="ignore"):
        delta = 6.0 * U32 * (np.abs(x) + abs(mx) + abs(ln_m))
        delta[~np.isfinite(delta)] = 0.0
        must = must & ((x >= mx + ln_m + delta) | (x == mx))
        may = may & (x >= mx + ln_m - delta)
    y = x + so.gumbel(seed, so.counter_base(row, counter, step), V)
    tok, margin = so._argmax_margin(y, may)
    tok_must, _ = so._argmax_margin(y, must)
    return so.RowOracle(tok, tok_must, margin, must, may, so.log_softmax64(x))


# ------------------------------------------------------------------ fixed cases
REPS = (1.0, 1.1, 1.5, 0.8)
FREQS = (0.0, 0.5, 2.0, -1.0)
PRESS = (0.0, 0.5, 2.0, -1.0)
MINPS = (0.0, 0.02, 0.3, 1.0)
# row -> slot: not the identity, slots shared by rows, some rows without one
ROW_SLOT = (3, -1, 0, 5, 1, 7, -1, 2, 6, 4, 3, 0, -1, 7, 5, 1, 2, 6, 4, -1, 3, 5, 7, 6, 4)
GREEDY_ROWS = (4, 13)               # penalised greedy rows (slots 1 and 7)
SHORT_SLOTS = (0, 1, 2)             # histories of length 0, 1 and 8
SHORT_REPS = {0: (0.8, 0.8), 1: (0.8, 1.1), 2: (1.1, 1.1)}   # per slot: its first, second row


def _row_reps():
    """Repetition penalty per row.  l / 0.8 = 1.25 l and l * 1.1 = 11 l / 10 land on (or, r being
    an fp32 number, within a few 2^-27 of) a bf16 midpoint often: over random bf16 logits about
    20 % of the positive ones are ambiguous at r = 0.8 and about 8.5 % of the negative ones at
    r = 1.1 (none of the other sign: 0.8 l and l / 1.1 stay clear of midpoints) - by
    construction, whatever the kernel does.  The caps on ambiguous elements and inexact rows are
    conditions, so the rows with 64-token histories take r in {1, 1.5} (1.5 l is exact in fp32,
    l / 1.5 is rounded but never near a midpoint), the two rows of the 8-token history take
    r = 1.1, and the rows with 0- and 1-token histories take 0.8 and 1.1."""
    out, seen, nl = [], {}, 0
    for s in ROW_SLOT:
        if s in SHORT_SLOTS:
            out.append(SHORT_REPS[s][seen.get(s, 0) % 2])
            seen[s] = seen.get(s, 0) + 1
        else:
            out.append((1.0, 1.5)[nl % 2])
            nl += 1
    return out


NEG_INF_SLOT = 6                    # its first prompt token gets a -inf logit in its rows


@dataclass
class Case:
    base: so.Case              # the matrix case of V (logits with the -inf elements set)
    V: int
    prompts: List[List[int]]   # per slot
    outputs: List[List[int]]   # per slot
    table: torch.Tensor        # int32 [SLOTS, V]
    pen_slot: torch.Tensor     # int32 [B]
    rep: torch.Tensor          # f32 [B]
    pres: torch.Tensor
    freq: torch.Tensor
    min_p: torch.Tensor


def _histories(V: int):
    """Per slot (prompt, outputs): lengths 0, 1, 8 and 64; repeats with counts up to 40; tokens 0
    and V - 1; tokens in the prompt only, in the outputs only and in both."""
    g = np.random.default_rng(7 + V)
    rnd = lambda n: [int(t) for t in g.integers(0, V, n)]
    both = rnd(4)
    prompts = [[],                                  # slot 0: no history at all
               [0],                                 # 1: length 1, prompt only
               rnd(3),                              # 2: length 8, prompt and outputs
               [0] + both + rnd(27),                # 3: 32 + 32, tokens in both
               rnd(8),                              # 4: one token generated 40 times
               rnd(48) + rnd(8) * 2,                # 5: prompt only, with duplicates
               rnd(40),                             # 6: holds the -inf logit (first token)
               [V - 1] + rnd(15)]                   # 7
    rep40 = rnd(1)
    outputs = [[],
               [],
               [V - 1] + rnd(4),
               both + [V - 1] + rnd(9) * 3,
               rep40 * 40 + rnd(16),
               [],
               rnd(12) * 2,
               [0] * 7 + rnd(41)]
    return prompts, outputs


@functools.lru_cache(maxsize=None)
def case(V: int) -> Case:
    b = so.matrix_case(V)
    B = b.logits.shape[0]
    assert B == len(ROW_SLOT)
    prompts, outputs = _histories(V)
    table = torch.from_numpy(np.stack([table_row(V, p, o) for p, o in zip(prompts, outputs)]))
    logits = b.logits.clone()
    temp = b.temperature.clone()
    for row in GREEDY_ROWS:
        temp[row] = 0.0
    for row, s in enumerate(ROW_SLOT):
        if s == NEG_INF_SLOT:
            logits[row, prompts[s][0]] = float("-inf")
    rows = range(B)
    base = so.Case(logits, temp, b.top_k, b.top_p, b.seeds, b.counters)
    return Case(base, V, prompts, outputs, table,
                torch.tensor(ROW_SLOT, dtype=torch.int32),
                torch.tensor(_row_reps()),
                torch.tensor([PRESS[(i // 2 + 1) % 4] for i in rows]),
                torch.tensor([FREQS[(i + i // 4) % 4] for i in rows]),
                torch.tensor([MINPS[(i + i // 4 + 2) % 4] for i in rows]))


@functools.lru_cache(maxsize=None)
def penalty_oracle(V: int) -> List[Optional[PenaltyOracle]]:
    """Per row of ``case(V)``: the oracle of the penalised row, None for rows without a slot."""
    c = case(V)
    lg = c.base.logits.double().numpy()
    tab = c.table.numpy().astype(np.int64)
    out = []
    for row, s in enumerate(ROW_SLOT):
        if s < 0:
            out.append(None)
            continue
        w = tab[s]
        out.append(penalise_row(lg[row], w < 0, w & 0x7FFFFFFF, float(c.rep[row]),
                                float(c.freq[row]), float(c.pres[row])))
    return out


@functools.lru_cache(maxsize=None)
def penalised_logits(V: int) -> torch.Tensor:
    """The oracle-penalised bf16 logits [B, V] (rows without a slot unchanged)."""
    c = case(V)
    out = c.base.logits.clone()
    for row, o in enumerate(penalty_oracle(V)):
        if o is not None:
            out[row] = o.expect
    return out


def _sample_rows(logits: torch.Tensor, c: Case, min_p) -> List[so.RowOracle]:
    b = c.base
    lg = logits.double().numpy()
    return [sample_row(lg[i], float(b.temperature[i]), int(b.top_k[i]), float(b.top_p[i]),
                       float(min_p[i]) if min_p is not None else 0.0, int(b.seeds[i]), row=i,
                       counter=int(b.counters[i])) for i in range(lg.shape[0])]


@functools.lru_cache(maxsize=None)
def token_oracle(V: int) -> List[so.RowOracle]:
    """apply -> sample: the sampler's oracle (min-p included) on the oracle-penalised logits."""
    c = case(V)
    return _sample_rows(penalised_logits(V), c, c.min_p)


@functools.lru_cache(maxsize=None)
def min_p_only_oracle(V: int) -> List[so.RowOracle]:
    """min-p alone: the sampler's oracle on the case's (unpenalised) logits."""
    c = case(V)
    return _sample_rows(c.base.logits, c, c.min_p)


def row_exact(V: int, row: int) -> bool:
    o = penalty_oracle(V)[row]
    return o is None or o.exact


def penalty_mismatches(got_row: torch.Tensor, orig_row: torch.Tensor, o: PenaltyOracle):
    """Indices at which a penalised row (bf16 or fp32, CPU) disagrees with the oracle: touched
    elements must be one of the accepted bf16 neighbours (bf16; the two coincide unless the
    element is ambiguous) or lie within E of the float64 value (fp32); every other element must
    be bit-identical to the input."""
    touched = torch.from_numpy(o.touched)
    if got_row.dtype == torch.bfloat16:
        g = got_row.view(torch.int16)
        ok_t = (g == o.lo.view(torch.int16)) | (g == o.hi.view(torch.int16))
        same = g == orig_row.view(torch.int16)
    else:
        v = torch.from_numpy(o.value)
        gd = got_row.double()
        ok_t = ((gd - v).abs() <= torch.from_numpy(o.bound)) | (gd == v)
        same = got_row.view(torch.int32) == orig_row.view(torch.int32)
    return torch.nonzero(~torch.where(touched, ok_t, same)).flatten().tolist()
