"""Forcing the rare branches of numpy's Generator(PCG64): CPU-only helper of the forced-RNG tests (Python ints + numpy).

PCG64 XSL-RR 128/64 steps state' = state * MULT + inc and outputs rotr64(hi ^ lo, hi >> 58) of state'.  Both are invertible in closed form,
so a state can be built whose next raw word is any chosen 64-bit value at any chosen rotation (forced_state); the buffered 32-bit half
(has_uint32 / uinteger) is part of the state and forces the next 32-bit draw directly.  classify replays a described draw sequence on
numpy's own Generator and names the branch each draw took from the number of words it consumed; find_seed / scan_seeds search ordinary
seeds for a branch at a given draw position (the ziggurat classes cannot be inverted past the first draw).

Words are in the layout of rng_state() / set_rng_state(): (state_hi, state_lo, inc_hi, inc_lo, has_uint32, uinteger).
"""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
PCG_MULT = (0x2360ED051FC65DA4 << 64) | 0x4385DF649FCCF645
PCG_MULT_INV = pow(PCG_MULT, -1, 1 << 128)
# default_rng(0)'s increment: any odd 128-bit value is a valid stream
DEFAULT_INC = int(np.random.PCG64(0).state["state"]["inc"])

_HEADER = Path(__file__).resolve().parent.parent / "include" / "kp1_ziggurat_tables.h"
R = float(re.search(r"#define\s+KP1_ZIGGURAT_NOR_R\s+([0-9.eE+-]+)", _HEADER.read_text()).group(1))

ONE_BELOW = (1 << 53) - 1    # k of the largest double below 1: random() = k * 2^-53


def rotl64(x: int, r: int) -> int:
    r &= 63
    return ((x << r) | (x >> ((64 - r) & 63))) & M64 if r else x & M64


def forced_state(word: int, inc: int, hi: int) -> int:
    """the 128-bit state whose NEXT step lands on (hi, lo) with output `word`: rot = hi >> 58, lo = rotl64(word, rot) ^ hi"""
    assert inc & 1 and 0 <= word <= M64 and 0 <= hi <= M64 and 0 < inc <= M128
    lo = rotl64(word, hi >> 58) ^ hi
    return ((((hi << 64) | lo) - inc) * PCG_MULT_INV) & M128


def words(state: int, inc: int, has_uint32: int = 0, uinteger: int = 0) -> np.ndarray:
    return np.array([state >> 64, state & M64, inc >> 64, inc & M64, has_uint32, uinteger], dtype=np.uint64)


def forced_words(word: int, *, hi: int, inc: int = DEFAULT_INC, has_uint32: int = 0, uinteger: int = 0) -> np.ndarray:
    return words(forced_state(word, inc, hi), inc, has_uint32, uinteger)


def double_word(k: int, low11: int = 0) -> int:
    """a raw word whose random() is k * 2^-53 (the low 11 bits are discarded by the draw)"""
    assert 0 <= k <= ONE_BELOW and 0 <= low11 < 2048
    return (k << 11) | low11


def k_of(u: float) -> int:
    """k with k * 2^-53 == u exactly (u a multiple of 2^-53 in [0, 1))"""
    k = int(u * (1 << 53))
    assert k * 2.0 ** -53 == u and 0 <= k <= ONE_BELOW
    return k


def seed_words(seed: int) -> np.ndarray:
    return words_of(np.random.PCG64(seed))


def words_of(bitgen) -> np.ndarray:
    st = bitgen.state
    return words(int(st["state"]["state"]), int(st["state"]["inc"]), int(st["has_uint32"]), int(st["uinteger"]))


def bitgen_of(w) -> np.random.PCG64:
    w = [int(x) for x in w]
    b = np.random.PCG64(0)
    b.state = {"bit_generator": "PCG64", "state": {"state": (w[0] << 64) | w[1], "inc": (w[2] << 64) | w[3]}, "has_uint32": w[4], "uinteger": w[5]}
    return b


def generator_of(w) -> np.random.Generator:
    return np.random.Generator(bitgen_of(w))


def lcg_steps(before, after, limit: int = 4096) -> int:
    """number of PCG64 steps from the state in `before` to the state in `after` (same stream)"""
    b, a = [int(x) for x in before], [int(x) for x in after]
    assert b[2:4] == a[2:4]
    s, inc, target = (b[0] << 64) | b[1], (b[2] << 64) | b[3], (a[0] << 64) | a[1]
    for n in range(limit + 1):
        if s == target:
            return n
        s = (s * PCG_MULT + inc) & M128
    raise ValueError("states further apart than the limit")


def lemire_threshold(n: int) -> int:
    return (1 << 32) % n


def lemire_rejected(n: int, *, skip: int = 0) -> int:
    """the (skip+1)-th smallest non-zero 32-bit value that Lemire's method rejects for a range of n (n no power of two)"""
    t = lemire_threshold(n)
    assert t > 0
    found = -1
    j = 1
    while True:
        v = -((-j << 32) // n)          # ceil(j * 2^32 / n): the first v whose product reaches the j-th multiple of 2^32
        if ((v * n) & 0xFFFFFFFF) < t:
            found += 1
            if found == skip:
                return v
        j += 1


def lemire_at_threshold(n: int) -> int:
    """a 32-bit value whose leftover (v * n mod 2^32) equals the threshold exactly: accepted, next to the rejected ones"""
    t = lemire_threshold(n)
    g = int(np.gcd(n, 1 << 32))
    assert t % g == 0
    v = (t // g) * pow(n // g, -1, (1 << 32) // g) % ((1 << 32) // g)
    assert (v * n) & 0xFFFFFFFF == t
    return int(v)


def classify(w, draws) -> list[tuple[str, int]]:
    """[(label, words consumed)] per draw of `draws` replayed with numpy's Generator from the state `w`.  Draw kinds: "double",
    ("integers", lo, hi_exclusive), "normal".  Labels: double -> "double"; integers -> "integers" / "lemire_reject"; normal -> "fast" /
    "wedge_accept" (2 words) / "wedge_reject" (>= 3 words, |z| <= R) / "tail" (|z| > R) / "tail_retry" (tail whose inner loop repeats)."""
    bg = bitgen_of(w)
    g = np.random.Generator(bg)
    out = []
    for d in draws:
        before = words_of(bg)
        if d == "double":
            g.random()
            out.append(("double", lcg_steps(before, words_of(bg))))
        elif d == "normal":
            z = float(g.standard_normal())
            n = lcg_steps(before, words_of(bg))
            raw = [int(x) for x in np.atleast_1d(bitgen_of(before).random_raw(n))]
            out.append((_normal_label(raw, z), n))
        else:
            _, lo, hi = d
            g.integers(lo, hi)
            after = words_of(bg)
            n = lcg_steps(before, after)
            halves = int(before[4]) + 2 * n - int(after[4])
            out.append(("lemire_reject" if halves > 1 else "integers", n))
    return out


def _normal_label(raw: list[int], z: float) -> str:
    """walk the words one standard_normal consumed: a head word that is not the last one left its fast path; layer 0 enters the tail loop
    (pairs of doubles until it returns), any other layer takes one more word for the wedge test"""
    i, rejected = 0, False
    while True:
        if i == len(raw) - 1:
            assert abs(z) <= R
            return "wedge_reject" if rejected else "fast"
        if raw[i] & 0xFF == 0:
            pairs, rem = divmod(len(raw) - 1 - i, 2)
            assert rem == 0 and pairs >= 1 and abs(z) > R
            return "tail_retry" if pairs > 1 else "tail"
        if i + 2 == len(raw):
            assert abs(z) <= R
            return "wedge_reject" if rejected else "wedge_accept"
        rejected = True
        i += 2


def scan_seeds(draws, wants, *, start: int = 0, limit: int = 2_000_000) -> dict[tuple[str, int], list[int]]:
    """one pass over the seeds start, start + 1, ...: wants = {(label, position): count} -> the first `count` seeds for each"""
    need = dict(wants)
    found: dict[tuple[str, int], list[int]] = {k: [] for k in wants}
    positions = sorted({at for _, at in wants})
    normal_only = all(draws[at] == "normal" for at in positions)
    for seed in range(start, start + limit):
        w = seed_words(seed)
        if normal_only and not _any_slow_normal(w, draws):
            continue
        labels = classify(w, draws)
        for at in positions:
            key = (labels[at][0], at)
            if need.get(key, 0) > 0:
                found[key].append(seed)
                need[key] -= 1
        if not any(need.values()):
            return found
    raise ValueError(f"not found within {limit} seeds: {need}")


def _any_slow_normal(w, draws) -> bool:
    """cheap pre-filter: does the sequence consume more words than its fast paths need?  (one word per double and per normal; the
    bounded integers take one 32-bit half each, two halves to a word, the first from the buffered half when the state holds one)"""
    bg = bitgen_of(w)
    g = np.random.Generator(bg)
    minimum = halves = 0
    for d in draws:
        if d == "double":
            g.random()
            minimum += 1
        elif d == "normal":
            g.standard_normal()
            minimum += 1
        else:
            g.integers(d[1], d[2])
            halves += 1 if d[2] - d[1] > 1 else 0
    minimum += (max(halves - int(w[4]), 0) + 1) // 2
    return lcg_steps(w, words_of(bg)) > minimum


def find_seed(draws, want: str, at: int, *, start: int = 0, limit: int = 2_000_000) -> int:
    """the first seed >= start whose default stream reaches class `want` at draw position `at`"""
    return scan_seeds(draws, {(want, at): 1}, start=start, limit=limit)[(want, at)][0]
