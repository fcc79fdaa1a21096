"""CPU oracle of the token sampler (csrc/kernels/sampling.hip), bit-exact in its random draw.

Written from the kernel's specification, independently of ``ops.reference.sample`` (whose random
stream differs from the kernel's):

* hash: ``r = splitmix64(seed ^ splitmix64(base + i))`` on uint64 with wraparound; ``base`` is
  ``counters[row] * 0x100000001B3`` or, without counters, ``(step * 0x100000001B3) ^ (row << 40)``;
  the default seed is 0x1234;
* uniform: the kernel's integer -> fp32 formula evaluated in numpy float32 (identical rounding);
  everything after it (the two logs, ``x = logit / T``) in float64;
* kept set on ``x = float(logit) * (1 / T)`` in float64: top-k keeps every element >= the k-th
  largest value (ties kept; off for k <= 0 or k >= V); top-p, within the top-k set of mass Z,
  keeps the smallest prefix of descending value groups whose mass reaches p * Z (ties kept;
  off for p >= 1; p <= 0 keeps the maximum value group).  The kernel sums fp32 ``__expf`` masses,
  so two sets are returned: ``must_keep`` (groups whose preceding mass is < p*Z*(1 - 1e-3)) and
  ``may_keep`` (the same with 1 + 1e-3);
* draw: argmax of ``x + g``, ``g = -log(-log(u))``, lowest index on ties, with the margin to the
  runner-up;
* log-probability: float64 ``log_softmax(x)[token]`` over the whole (unfiltered) row.

A row is *decisive* when the argmax over ``must_keep`` equals the one over ``may_keep`` and its
margin exceeds ``MARGIN``: then the kernel has to return exactly that token.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
MUL1 = np.uint64(0xBF58476D1CE4E5B9)
MUL2 = np.uint64(0x94D049BB133111EB)
CTR_MUL = 0x100000001B3
DEFAULT_SEED = 0x1234
M64 = (1 << 64) - 1

UNIFORM_BITS = 23      # random bits per uniform: (2n + 1) < 2^24 is exact in fp32
BAND = 1e-3            # relative band around the fp32 top-p mass target (a condition, not a fit)
MARGIN = 1e-2          # least margin of a decisive row (a condition, not a fit)

# an all-ones raw draw (the largest uniform): seed, counter, element index at V = 128256
ALL_ONES_TRIPLE = (3, 228, 128165)
ALL_ONES_V = 128256


def _u64(x) -> np.ndarray:
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.asarray(int(x) & M64, dtype=np.uint64)


def splitmix64(x) -> np.ndarray:
    """One splitmix64 output for the state(s) ``x`` (uint64, wraparound)."""
    x = _u64(x)
    with np.errstate(over="ignore"):
        x = x + GOLDEN
        x = (x ^ (x >> np.uint64(30))) * MUL1
        x = (x ^ (x >> np.uint64(27))) * MUL2
        return x ^ (x >> np.uint64(31))


def counter_base(row: int, counter: Optional[int] = None, step: int = 0) -> int:
    if counter is not None:
        return (int(counter) * CTR_MUL) & M64
    return ((int(step) * CTR_MUL) & M64) ^ ((int(row) << 40) & M64)


def raw_draws(seed: int, base: int, n: int, start: int = 0) -> np.ndarray:
    """The 64-bit hash of elements ``start .. start + n - 1`` of a row."""
    with np.errstate(over="ignore"):
        ctr = np.asarray(base & M64, dtype=np.uint64) + np.arange(start, start + n, dtype=np.uint64)
    return splitmix64(_u64(seed) ^ splitmix64(ctr))


def uniform_from_raw(r) -> np.ndarray:
    """The kernel's ``uniform01`` of the raw 64-bit draw(s) ``r``, in float32."""
    n = (_u64(r) >> np.uint64(64 - UNIFORM_BITS)).astype(np.float32)
    return (n + np.float32(0.5)) * np.float32(1.0 / (1 << UNIFORM_BITS))


def gumbel(seed: int, base: int, n: int) -> np.ndarray:
    u = uniform_from_raw(raw_draws(seed, base, n)).astype(np.float64)
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(u))


def scaled(logits_row, temperature: float) -> np.ndarray:
    """``x = float(logit) * (1 / T)`` in float64 (``T`` as the fp32 value the kernel reads)."""
    x = np.asarray(logits_row, dtype=np.float64)
    return x * (1.0 / float(np.float32(temperature)))


def kept_sets(x: np.ndarray, top_k: int = 0, top_p: float = 1.0):
    """(must_keep, may_keep) boolean masks over ``x`` (float64, already divided by T)."""
    V = x.shape[0]
    xs = np.sort(x)[::-1]
    n_k = V
    if 0 < top_k < V:
        # every element >= the k-th largest value: xs is descending, -xs ascending
        n_k = int(np.searchsorted(-xs, -xs[top_k - 1], side="right"))
    thr_k = xs[n_k - 1]
    p = float(np.float32(top_p))
    if not p < 1.0:
        m = x >= thr_k
        return m, m.copy()
    xk = xs[:n_k]
    with np.errstate(invalid="ignore"):
        mass = np.exp(xk - xk[0])
    mass[np.isnan(mass)] = 0.0          # -inf - -inf on a row of -inf only
    cum = np.cumsum(mass)
    z = cum[-1]
    # mass preceding each element's value group (all elements of a tie share the group's start)
    start = np.searchsorted(-xk, -xk, side="left")
    before = (cum - mass)[start]
    out = []
    for band in (1.0 - BAND, 1.0 + BAND):
        keep = before < p * z * band
        keep[start == 0] = True          # the maximum value group is always kept (also p <= 0)
        thr = xk[int(np.nonzero(keep)[0][-1])]
        out.append(x >= thr)
    return out[0], out[1]


def _argmax_margin(y: np.ndarray, mask: np.ndarray):
    idx = np.nonzero(mask)[0]
    ym = y[idx]
    j = int(np.argmax(ym))              # first maximum = lowest index
    best = ym[j]
    if ym.shape[0] == 1:
        return int(idx[j]), float("inf")
    rest = np.delete(ym, j)
    second = rest.max()
    margin = float("inf") if second == -np.inf else float(best - second)
    return int(idx[j]), margin


@dataclass
class RowOracle:
    token: int            # argmax over may_keep
    token_must: int       # argmax over must_keep
    margin: float         # best - second best perturbed value over may_keep
    must_keep: np.ndarray
    may_keep: np.ndarray
    logprobs: np.ndarray  # float64 log_softmax(x) of the whole row

    @property
    def decisive(self) -> bool:
        return self.token == self.token_must and self.margin > MARGIN


def log_softmax64(x: np.ndarray) -> np.ndarray:
    mx = x.max()
    return x - mx - np.log(np.exp(x - mx).sum())


def sample_row(logits_row, temperature: float, top_k: int = 0, top_p: float = 1.0,
               seed: int = DEFAULT_SEED, row: int = 0, counter: Optional[int] = None,
               step: int = 0) -> RowOracle:
    lg = np.asarray(logits_row, dtype=np.float64)
    V = lg.shape[0]
    if not temperature > 0:
        # greedy: first maximum of the logits, log-probability under softmax(logits)
        tok = int(np.argmax(lg))
        only = np.zeros(V, dtype=bool)
        only[tok] = True
        return RowOracle(tok, tok, float("inf"), only, only.copy(), log_softmax64(lg))
    x = scaled(lg, temperature)
    must, may = kept_sets(x, int(top_k), float(top_p))
    finite = x > -np.inf                 # a -inf logit has no mass: in no support (unless all are)
    if finite.any():
        must, may = must & finite, may & finite
    y = x + gumbel(seed, counter_base(row, counter, step), V)
    tok, margin = _argmax_margin(y, may)
    tok_must, _ = _argmax_margin(y, must)
    return RowOracle(tok, tok_must, margin, must, may, log_softmax64(x))


def sample_rows(logits: torch.Tensor, temperature, top_k=None, top_p=None, seeds=None,
                counters=None, step: int = 0):
    """Oracle of every row of ``logits`` [B, V] (any float dtype; parameters are sequences)."""
    lg = logits.double().numpy()
    out = []
    for b in range(lg.shape[0]):
        out.append(sample_row(
            lg[b], float(temperature[b]),
            int(top_k[b]) if top_k is not None else 0,
            float(top_p[b]) if top_p is not None else 1.0,
            int(seeds[b]) if seeds is not None else DEFAULT_SEED,
            row=b, counter=int(counters[b]) if counters is not None else None, step=step))
    return out


# ------------------------------------------------------------------ shared inputs of the tests
# vocabularies at every dispatch edge of launch_sample and of the vector loops: tiny, element-wise
# (odd), NV 4 -> 8, NV 8 -> 16, Llama-3, NV 16 -> radix for bf16
VOCABS = (8, 1000, 1003, 32768, 32776, 65536, 65544, 128256, 131072, 131080)
MAX_NON_DECISIVE = 0.05


@dataclass
class Case:
    logits: torch.Tensor       # [B, V] bf16 (CPU)
    temperature: torch.Tensor  # [B] f32
    top_k: torch.Tensor        # [B] i32
    top_p: torch.Tensor        # [B] f32
    seeds: torch.Tensor        # [B] i64
    counters: torch.Tensor     # [B] i64


@functools.lru_cache(maxsize=None)
def matrix_case(V: int) -> Case:
    """24 rows scaled like test_sample_register_path_matches_radix_path (every top-k x top-p
    pair once) plus one row with top_p = 0 (keep the maximum value group)."""
    g = torch.Generator().manual_seed(1000003 + V)
    B = 25
    scale = torch.cat([torch.linspace(0.5, 6, 24), torch.tensor([2.0])])
    logits = (torch.randn(B, V, generator=g) * scale[:, None]).to(torch.bfloat16)
    t = torch.cat([torch.linspace(0.3, 1.5, 24), torch.tensor([0.8])])
    ks = torch.tensor([0, 1, 2, 5, 40, 1000, V - 1, V] * 3 + [0], dtype=torch.int32)
    ps = torch.tensor([1.0, 0.99, 0.9, 0.7, 0.5, 0.1] * 4 + [0.0])
    seeds = torch.arange(B, dtype=torch.int64) * 7919 + 3 + V
    ctr = torch.arange(B, dtype=torch.int64) * 13 + 100
    return Case(logits, t, ks, ps, seeds, ctr)


@functools.lru_cache(maxsize=None)
def matrix_oracle(V: int):
    c = matrix_case(V)
    return sample_rows(c.logits, c.temperature, c.top_k, c.top_p, c.seeds, c.counters)


STEP_V, STEP = 128256, 77


@functools.lru_cache(maxsize=None)
def step_oracle():
    """The matrix case of STEP_V keyed by (step, row) instead of per-row counters."""
    c = matrix_case(STEP_V)
    return sample_rows(c.logits, c.temperature, c.top_k, c.top_p, c.seeds, None, step=STEP)


MIXED_V = 32776


@functools.lru_cache(maxsize=None)
def mixed_case():
    """The matrix case of MIXED_V with every third row greedy (T = 0)."""
    c = matrix_case(MIXED_V)
    t = c.temperature.clone()
    t[::3] = 0.0
    return Case(c.logits, t, c.top_k, c.top_p, c.seeds, c.counters)


@functools.lru_cache(maxsize=None)
def mixed_oracle():
    c = mixed_case()
    return sample_rows(c.logits, c.temperature, c.top_k, c.top_p, c.seeds, c.counters)


def all_ones_logits() -> torch.Tensor:
    """One row of -30 with a single 0 at index 7: every draw but an infinite one picks 7."""
    lg = torch.full((1, ALL_ONES_V), -30.0)
    lg[0, 7] = 0.0
    return lg


def support_rows():
    """Constructed rows of V = 64 (values exact in bf16) for the support test: (name, logits,
    top_k, top_p).  Masses are well separated, with a three-way tie straddling the top-k cut
    and another straddling the top-p cut; every kept token has probability >= 0.02 of the kept
    mass and the cuts are far from the band, so must_keep == may_keep."""
    rows = []
    # top-k = 4 cuts inside the tie {1.0, 1.0, 1.0} at ranks 3..5: all three stay (5 kept)
    a = torch.full((64,), -8.0)
    a[[5, 17, 40, 41, 63]] = torch.tensor([2.0, 1.5, 1.0, 1.0, 1.0])
    a[[0, 9]] = torch.tensor([0.5, 0.0])
    rows.append(("topk_tie", a, 4, 1.0))
    # top-p = 0.6: mass e^2 : e^1.5 : 3 x e^1 ...; 0.6 * Z falls inside the tie, which stays whole
    b = torch.full((64,), -8.0)
    b[[3, 11, 30, 31, 62]] = torch.tensor([2.0, 1.5, 1.0, 1.0, 1.0])
    b[[1, 20, 50]] = torch.tensor([-1.0, -1.5, -2.0])
    rows.append(("topp_tie", b, 0, 0.6))
    # both filters, and -inf logits (never sampled) among the rest
    c = torch.full((64,), float("-inf"))
    c[[2, 8, 16, 32, 33, 34, 60]] = torch.tensor([1.0, 0.5, 0.0, -0.5, -0.5, -0.5, -3.0])
    rows.append(("neg_inf", c, 6, 0.95))
    # no filter: the support is every finite logit
    d = torch.full((64,), float("-inf"))
    d[[0, 7, 21, 63]] = torch.tensor([0.0, -1.0, -2.0, -3.0])
    rows.append(("neg_inf_unfiltered", d, 0, 1.0))
    return rows
