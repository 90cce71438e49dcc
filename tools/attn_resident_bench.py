#!/usr/bin/env python3
"""Cross-attention forward over a long prompt's keys (154 / 231: two / three 75-token windows of clip_text.encode_tokens): the
LDS-resident kernel (SKG_ATTN_RESIDENT_KV) against the streaming flash kernel, same call with and without the flag, in
alternating rounds in one process.  Shapes: the cross-attentions of an SD1.5 training batch of 4 rows and of a sampling batch of
8 x 2 rows (8 heads of 40 / 80 / 160 over 4096 / 1024 / 256 queries), and SD2.x's heads of 64.  Prints the table kept as
profiles/attn_resident_kv.txt: median, min and max of the rounds per form, the gain of the medians, and whether the gain
exceeds the spread of the rounds (the routing rule of unet._RESIDENT_KV)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sketch2img_amd import ops  # noqa: E402

DEV = "cuda:0"


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters          # us per call


def case(rows, heads, N, dh, Nkv, rounds, iters):
    C, kvs, scale = heads * dh, (Nkv + 7) // 8 * 8, dh ** -0.5
    g = torch.Generator(device=DEV).manual_seed(rows + N + dh + Nkv)
    q = torch.randn(rows * N, C, device=DEV, generator=g).half()
    kv = torch.zeros(rows, kvs, 2 * C, device=DEV, dtype=torch.float16)
    kv[:, :Nkv] = torch.randn(rows, Nkv, 2 * C, device=DEV, generator=g).half()
    kv = kv.view(rows * kvs, 2 * C)
    k, v = kv[:, :C], kv[:, C:]
    out = torch.empty(rows * N, C, device=DEV, dtype=torch.float16)
    forms = {f: (lambda f=f: ops.attn_fwd(q, k, v, rows, heads, N, Nkv, kvs, dh, scale, out=out, want_lse=True, v_rows=True,
                                           resident_kv=f)) for f in (True, False)}
    o1 = forms[True]()[0].float()
    o0 = forms[False]()[0].float()
    diff = float((o1 - o0).norm() / o0.norm())
    for f in forms.values():
        window(f, iters)                               # warm-up of both forms
    t = {True: [], False: []}
    for _ in range(rounds):
        for f in (True, False):
            t[f].append(window(forms[f], iters))
    med = {f: statistics.median(t[f]) for f in t}
    spread = max(max(t[f]) - min(t[f]) for f in t)
    gain = med[False] - med[True]
    tiles = 10 if kvs <= 160 else 15
    verdict = "resident" if gain > spread else ("streaming" if -gain > spread else "tie")
    print(f"rows {rows:2d} heads {heads:2d} d {dh:3d} Nq {N:4d} keys {Nkv:3d} tiles {tiles:2d} | resident {med[True]:7.1f} "
          f"[{min(t[True]):7.1f} {max(t[True]):7.1f}] | streaming {med[False]:7.1f} [{min(t[False]):7.1f} {max(t[False]):7.1f}] us | "
          f"gain {gain:+7.1f} us ({100 * gain / med[False]:+5.1f} %) spread {spread:5.1f} -> {verdict} | rel diff {diff:.1e}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    print(torch.cuda.get_device_name(0), f"| {a.rounds} alternating rounds of {a.iters} calls; [min max] over the rounds")
    for rows in (4, 16):
        for heads, N, dh in ((8, 4096, 40), (8, 1024, 80), (8, 256, 160), (8, 64, 160), (5, 4096, 64), (10, 1024, 64), (20, 256, 64)):
            for Nkv in (154, 231):
                case(rows, heads, N, dh, Nkv, a.rounds, a.iters)
