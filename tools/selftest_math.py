#!/usr/bin/env python3
"""Exhaustive verification of the lean division / square root (sdirt_device.hpp: Lean)
against the compiler's correctly rounded sequences, on the GPU.
  division: all 2^46 (mantissa_a, mantissa_b) pairs, operands in [1,2)   (~2.5 min)
  sqrt    : every fp32 with exponent in [-100, 128)                      (~0.5 s)
  sqrt_pos: every fp32 in [2^-100, 2^100]                                (~0.5 s)
and of the sag's a / sqrt_pos(1 - a) seeded with the root's v_rsq_f32 against the same division seeded with
v_rcp_f32 of the root, with the expression that reads it, on every fp32 a   (~0.5 s)
and of the sag's n / onesf^2 seeded with the square of the refined 1 / onesf against v_rcp_f32(onesf^2): the divisors
whose refined reciprocal differs, under every numerator mantissa             (~0.1 s)
  --seed2        that last check alone
  --seed2-full   ... and then ALL 2^23 + 1 divisors of [1, 2] under all 2^23 numerators   (~1 min)
and of that first quotient, seeded with v_rsq_f32, with and without the two fma that refine the seed, with the
expression that reads it, on every fp32 a                                    (~0.5 s)
  --seed-once    that last check alone (kept in profiles/sag_seed3/selftest_seed_once.txt)
Output is kept in profiles/rNN/selftest_math.txt."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sdirt_amd import _lib
from sdirt_amd.basics import dptr, stream_ptr

dev = torch.device("cuda:0")
h = _lib.lib()
out = torch.zeros(9, dtype=torch.int64, device=dev)


def run(mode, first, count, span=0):
    _lib.check(h.sdirt_selftest_math(mode, first, count, span, dptr(out), stream_ptr(dev)))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return int(o[0]), [hex(int(v) & 0xFFFFFFFFFFFFFFFF) for v in o[1:4]]


def pat(e):
    return (e + 127) << 23




def seed2():
    """mode 5; returns the misses as (onesf bits, numerator bits) pairs."""
    big = torch.zeros(64 + 4096, dtype=torch.int64, device=dev)
    t0 = time.time()
    _lib.check(h.sdirt_selftest_math(5, 0, (1 << 23) + 1, 0, dptr(big), stream_ptr(dev)))
    torch.cuda.synchronize()
    o = [int(v) & 0xFFFFFFFFFFFFFFFF for v in big.cpu().numpy()]
    members = sorted(o[64:64 + min(o[1], 4096)])
    misses = sorted((v >> 32, v & 0xFFFFFFFF) for v in o[4:4 + min(o[3], 16)])
    print(f"sag seed 2 (square of the refined 1/onesf for v_rcp of onesf^2): onesf checked {o[0]:#x}; refined reciprocal "
          f"differs |E| = {o[1]}: {[hex(v) for v in members]}; pairs checked {o[2]:#x}; quotient differs: {o[3]} "
          f"{[(hex(a), hex(b)) for a, b in misses]}   {time.time() - t0:.1f} s", flush=True)
    if "--seed2-full" not in sys.argv:
        return
    t0 = time.time()
    checked = bad = 0
    found = set()
    for first in range(0, (1 << 23) + 1, 4096):
        n = min(4096, (1 << 23) + 1 - first)
        _lib.check(h.sdirt_selftest_math(5, first, n, 1, dptr(big), stream_ptr(dev)))
        o = [int(v) & 0xFFFFFFFFFFFFFFFF for v in big[:20].cpu().numpy()]
        assert o[0] == n == o[1] and o[2] == n << 23, o[:4]
        checked += o[2]
        bad += o[3]
        found.update((v >> 32, v & 0xFFFFFFFF) for v in o[4:4 + min(o[3], 16)])
        if first % (1 << 20) == 0:
            print(f"  full scan: divisors up to {first + n:#x}, pairs {checked:#x}, differing {bad}", flush=True)
    print(f"sag seed 2, ALL (2^23 + 1) x 2^23 pairs: checked {checked:#x}; quotient differs: {bad} "
          f"{sorted((hex(a), hex(b)) for a, b in found)}   ({time.time() - t0:.0f} s)")


def seed_once():
    """mode 6; returns the decoded counts (_lib.decode_seed_once)."""
    big = torch.zeros(_lib.SELFTEST_LIST_WORDS + _lib.SELFTEST_LIST_CAP, dtype=torch.int64, device=dev)
    t0 = time.time()
    _lib.check(h.sdirt_selftest_math(6, 0, 1 << 32, 0, dptr(big), stream_ptr(dev)))
    torch.cuda.synchronize()
    s = _lib.decode_seed_once(big.cpu().numpy())
    first = ["none" if v is None else f"{v:#010x}" for v in s["first_g"]]
    print(f"sag seed, refined twice against not refined (a * r, one residual step by r), every fp32 a: checked "
          f"{s['checked']:#x}; G differs, 1 - a positive normal, a >= 0: {s['g_pos']} (first a {first[0]}); a < 0: "
          f"{s['g_neg']} (first a {first[1]}); G differs elsewhere, not NaN under both: {s['g_outside']} (first a "
          f"{first[2]}); bare quotient differs: {s['n_quot']}, the first 16: {[f'{v:#010x}' for v in s['quot'][:16]]}; "
          f"v_rsq_f32(1 - a) at a = {_lib.SEED_ONCE_PROBE:#010x}: {s['seed_bits']:#010x}, {s['seed_offset']:+d} floats "
          f"from the correctly rounded one   {time.time() - t0:.1f} s", flush=True)
    if s["n_quot"] > 16:
        print(f"  all {len(s['quot'])} listed: {[f'{v:#010x}' for v in s['quot']]}", flush=True)
    return s


if "--seed2" in sys.argv or "--seed2-full" in sys.argv:
    seed2()
    sys.exit(0)
if "--seed-once" in sys.argv:
    seed_once()
    sys.exit(0)
t = time.time()
print("sqrt, every fp32 in [2^-100, inf):", run(0, pat(-100), 0x7F800000 - pat(-100)),
      f"{time.time() - t:.1f} s")
print("sqrt, +0 / +inf / NaN / -0 / negatives:", run(0, 0, 1), run(0, 0x7F800000, 1),
      run(0, 0x7FC00000, 1), run(0, 0x80000000, 1), run(0, 0x80800000, 0xFF800001 - 0x80800000))
t = time.time()
print("sqrt_pos (rsq + Markstein), every fp32 in [2^-100, 2^100]:", run(3, 0, 1 << 32),
      f"{time.time() - t:.1f} s")
t = time.time()
_lib.check(h.sdirt_selftest_math(4, 0, 1 << 32, 0, dptr(out), stream_ptr(dev)))
torch.cuda.synchronize()
o = [int(v) & 0xFFFFFFFFFFFFFFFF for v in out.cpu().numpy()]
first = ["none" if v == 0xFFFFFFFFFFFFFFFF else f"{v:#010x}" for v in o[4:7]]
print(f"sag seed (v_rsq of the radicand for v_rcp of the root), every fp32 a: checked {o[0]:#x}; "
      f"G differs, 1 - a positive normal: {o[1]} (first a {first[0]}); G differs elsewhere, not NaN under both: {o[2]} "
      f"(first a {first[1]}); bare quotient differs: {o[3]} (first a {first[2]})   {time.time() - t:.1f} s")
seed2()
seed_once()
t = time.time()
total = 0
step = 1 << 42
for k in range(0, 1 << 46, step):
    n, ex = run(2, k, step)
    total += n
    print(f"div, mantissa pairs [{k:#x}, {k + step:#x}): mismatches {n} {ex if n else ''}", flush=True)
print(f"div, ALL 2^46 mantissa pairs: mismatches {total}   ({time.time() - t:.0f} s)")
print("div, 2^38 random pairs, exponents within +-40, random signs:", run(1, 0, 1 << 38, 40))
