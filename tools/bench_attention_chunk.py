#!/usr/bin/env python3
"""Query-block attention over the per-head cache (F5, paged_attention_kvc_chunk) against the only other way this
package can produce the same result: nq successive calls of the decode op with trimmed context lengths.

Llama-3-8B heads (32 query / 8 KV, head size 128, block size 16), batch 16, contexts 4k and 32k, nq 16 / 64 / 256,
with and without the metric, in both block layouts.  Times are medians of device-event timings after warm-up; the
algorithmic traffic of the chunk op is 2 * hd * e bytes per visible slot and query tile (16 tokens), reported as a
fraction of 8 TB/s.  Run on the GPU box:  python tools/bench_attention_chunk.py [--json out.json] [--only ctx,nq]

--kv-cache-dtype fp8_e4m3 / fp8_e5m2: the same over an fp8 cache (1 byte per element, unit scales -- the decode op's
fastest fp8 path).  The decode baseline then reads the fp8 cache too, and the chunk op over a 2-byte cache of the same
geometry is timed in the same process, its launches alternating with the fp8 ones (chunk_auto_ms).

--nq 1,2,4,8: short query blocks (draft verification).  schedule="short" against schedule="tile", launches alternating
in one process, and both against decode x nq; batch 16 at contexts 4k and 32k, one line each for batch 1 and batch 64
at 4k.  The traffic is then counted per CALL (2 * hd * e bytes per visible slot, read once), and the largest
difference between the two schedules' outputs is recorded next to the times.  With --kv-cache-dtype fp8_*: the two
schedules and the decode calls read the fp8 cache, and a third alternating leg times the short schedule over the
2-byte cache of the same geometry (short_auto_ms; fp8_short_over_auto_short is the ratio of the two medians).

--nq 16,32,64,128: query blocks with more than 32 rows per KV head in every configuration.  schedule="split" against
schedule="tile", batches of 4 launches of one schedule between a pair of events, the two schedules in turn, medians of
40 batches; the same grid (both layouts, with and without the metric, batch 1 and 64 at 4k / nq 16), over the fp8 cache
with --kv-cache-dtype fp8_*.  Traffic as in the first leg (per visible slot and query tile), the partition length the
library chose and the largest difference between the two schedules' outputs are recorded next to the times.

--wide --nq 5,6,8 --heads 70b (Llama-3-70B heads, 64 query / 8 KV) or --wide --nq 9,12,16 (8B heads): 33 .. 64 rows per KV
head.  schedule="wide" against schedule="tile" and schedule="split", launches as in the split leg (batches of 4 between
a pair of events, the three schedules in turn, medians of 40); both layouts without the metric, one row with the metric
per context, batch 1 and 64 at 4k for the first nq.  The traffic is counted per CALL as in the short leg, and the
largest difference between the wide and the tile outputs is recorded next to the times.  With --kv-cache-dtype fp8_* the
three schedules read the fp8 cache, and a fourth alternating leg times the wide schedule over the 2-byte cache of the
same geometry (wide_auto_ms; fp8_wide_over_auto_wide is the ratio of the two medians).

--metric-schedule tile|rows|both with --nq (at most 64 rows per KV head; --wide for 33 .. 64): the metric passes behind
ONE output schedule ("short" up to 32 rows, "wide" beyond).  The call without the metric, with metric_schedule="tile"
and with metric_schedule="rows" in turn (batches of 4 launches between a pair of events, medians of 40); a metric pass
is its call minus the call without the metric, its traffic the K bytes of the call (hd * e per slot).  Both layouts,
batch 16 at both contexts, batch 1 and 64 at 4k for the first nq; the largest relative difference between the two
metrics (from zeros) is recorded next to the times.

--tree --nq 7,15 (8B heads) or --tree --nq 7 --heads 70b (at most 64 rows per KV head): draft-TREE verification.  The
tree is fixed: nq nodes in heap order, node j's parent is (j - 1) // 2 -- complete binary trees at nq 7 (4 leaves, paths
of 3) and nq 15 (8 leaves, paths of 4).  One call with tree_mask (the nodes' ancestor words) against the chain call of
the same shape and nq, and against what a caller without tree_mask has to run: one chain call per root-to-leaf path, each
over the prefix plus the path's nodes.  The four legs -- tree, chain, the chain call a second time, the per-path calls --
in turn, batches of 4 launches between a pair of events, medians of 40; chain_again_over_chain is the spread a ratio of
two legs has by itself.  Both layouts without the metric, one row with the metric (row form on every side) per
context; over the fp8 cache with --kv-cache-dtype fp8_*."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import vllm_kvcompress_amd as kvc  # noqa: E402
from vllm_kvcompress_amd import _custom_ops as ops  # noqa: E402
from vllm_kvcompress_amd import _lib  # noqa: E402

S, HQ, HKV, HD, BS, TILE, PEAK = 16, 32, 8, 128, 16, 16, 8e12


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def timed_alternating(*fns, warmup, reps, batch=1):
    """the given calls in turn, `batch` launches of one between a pair of events (what else runs on the machine hits all
    alike) -> a (median, min, max) of the time per launch each"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = tuple([] for _ in fns)
    for _ in range(reps):
        for fn, acc in zip(fns, ms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(batch):
                fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b) / batch)
    return tuple((statistics.median(m), min(m), max(m)) for m in ms)


def make_cache(ctx, dev, gen, kvd="auto"):
    nblk = (ctx + BS - 1) // BS
    NB = S * HKV * nblk
    kc = torch.randn((NB, HD // 8, BS, 8), device=dev, generator=gen, dtype=torch.float16)
    vc = torch.randn((NB, HD, BS), device=dev, generator=gen, dtype=torch.float16)
    kc8 = vc8 = None
    if kvd != "auto":                  # N(0, 1) through the saturating cast: no NaN / inf byte; K [NB, hd/16, bs, 16]
        tf8 = torch.float8_e5m2 if kvd == "fp8_e5m2" else torch.float8_e4m3fn
        kc8 = kc.view(NB, HD // 16, BS, 16).to(tf8).view(torch.uint8)
        vc8 = vc.to(tf8).view(torch.uint8)
    bt = torch.randperm(NB, device=dev, generator=gen).to(torch.int32).view(S, HKV, nblk)
    lens = torch.full((S, HKV), ctx, dtype=torch.int32, device=dev)
    # positions: slot i of every head holds token i (an uncompressed history: every slot inside the window)
    pos = torch.zeros((NB, BS), dtype=torch.int32, device=dev)
    pos[bt.long().view(-1)] = torch.arange(nblk * BS, dtype=torch.int32, device=dev).view(1, nblk, BS).expand(
        S * HKV, nblk, BS).reshape(-1, BS)
    return kc, vc, bt, lens, pos, kc8, vc8


def run_tree(ctx, nq, with_metric, state, dev, gen, kvd):
    """one tree call of nq nodes against the chain call of the same shape, and against the per-path chain calls"""
    kc, vc, bt, lens, pos, kc8, vc8 = state
    fp8 = kvd != "auto"
    cache = (kc8, vc8) if fp8 else (kc, vc)
    kw = dict(kv_cache_dtype=kvd, k_scale=1.0, v_scale=1.0) if fp8 else {}
    rows = nq * (HQ // HKV)
    name = "wide" if rows > 32 else "short"
    scale = HD ** -0.5
    buf = torch.zeros(S, dtype=torch.int32, device=dev)
    metrics = torch.zeros(pos.shape, dtype=torch.float32, device=dev) if with_metric else None
    # the tree: nodes in heap order, node j's parent is (j - 1) // 2 -- complete binary trees at nq 7 (4 leaves, 3 levels)
    # and 15 (8 leaves, 4 levels); a node's word is its parent's plus its own bit, its position the prefix plus its depth
    words, depth = [], []
    for j in range(nq):
        words.append((words[(j - 1) // 2] if j else 0) | (1 << j))
        depth.append(depth[(j - 1) // 2] + 1 if j else 0)
    paths = [[i for i in range(nq) if (words[j] >> i) & 1] for j in range(nq) if 2 * j + 1 >= nq]
    q = torch.randn((S, nq, HQ, HD), device=dev, generator=gen, dtype=torch.float16)

    def call(nodes, tree):
        """the call that verifies these nodes of every sequence: as a tree (their words), or as a chain (a path)"""
        d = len(nodes)
        qn = q[:, nodes].reshape(S * d, HQ, HD).contiguous()
        out = torch.empty_like(qn)
        qsl = torch.arange(0, S * d + 1, d, dtype=torch.int32, device=dev)
        steps = [depth[j] for j in nodes] if tree else list(range(d))
        qpos = (torch.tensor(steps, dtype=torch.int32, device=dev) + (ctx - nq)).repeat(S)
        clens = (lens - (nq - d)).contiguous()
        mask = torch.tensor([words[j] for j in nodes], dtype=torch.int64, device=dev).repeat(S) if tree else None
        sched = "wide" if d * (HQ // HKV) > 32 else "short"
        return lambda: ops.paged_attention_kvc_chunk(
            out, qn, *cache, HKV, scale, bt, clens, pos, qsl, qpos, buf, BS, ctx - (nq - d), d, metrics=metrics, use_l2=True,
            schedule=sched, metric_schedule="rows", tree_mask=mask, **kw)

    tree_fn, chain_fn = call(list(range(nq)), True), call(list(range(nq)), False)
    path_fns = [call(p, False) for p in paths]

    def all_paths():
        for fn in path_fns:
            fn()

    # the chain call twice: the ratio of its two legs is the spread a ratio of this table has by itself
    (t_ms, t_lo, t_hi), (c_ms, c_lo, c_hi), (c2_ms, c2_lo, c2_hi), (p_ms, p_lo, p_hi) = timed_alternating(
        tree_fn, chain_fn, chain_fn, all_paths, warmup=5, reps=40, batch=4)
    return dict(layout=kvc.block_layout(), heads=[HQ, HKV], kv_cache_dtype=kvd, batch=S, ctx=ctx, nq=nq, rows=rows,
                schedule=name, metrics=with_metric, tree="binary, heap order", paths=len(paths), path_len=len(paths[0]),
                tree_ms=t_ms, tree_ms_min=t_lo, tree_ms_max=t_hi, chain_ms=c_ms, chain_ms_min=c_lo, chain_ms_max=c_hi,
                chain_again_ms=c2_ms, chain_again_ms_min=c2_lo, chain_again_ms_max=c2_hi,
                per_path_chain_calls_ms=p_ms, per_path_chain_calls_ms_min=p_lo, per_path_chain_calls_ms_max=p_hi,
                tree_over_chain=t_ms / c_ms, chain_again_over_chain=c2_ms / c_ms, paths_over_tree=p_ms / t_ms)


def run(ctx, nq, with_metric, state, dev, gen, kvd="auto", short=False, split=False, wide=False, metric_leg=None):
    kc, vc, bt, lens, pos, kc8, vc8 = state
    fp8 = kvd != "auto"
    dkc, dvc = (kc8, vc8) if fp8 else (kc, vc)          # what the decode baseline reads
    T = S * nq
    q = torch.randn((T, HQ, HD), device=dev, generator=gen, dtype=torch.float16)
    out = torch.empty_like(q)
    qsl = torch.arange(0, T + 1, nq, dtype=torch.int32, device=dev)
    qpos = (torch.arange(nq, dtype=torch.int32, device=dev) + (ctx - nq)).repeat(S)
    buf = torch.zeros(S, dtype=torch.int32, device=dev)
    metrics = torch.zeros(pos.shape, dtype=torch.float32, device=dev) if with_metric else None
    scale = HD ** -0.5

    def chunk(schedule="tile", out=out, metrics=metrics, metric_schedule="tile"):
        ops.paged_attention_kvc_chunk(out, q, kc, vc, HKV, scale, bt, lens, pos, qsl, qpos, buf, BS, ctx, nq,
                                      metrics=metrics, use_l2=True, schedule=schedule, metric_schedule=metric_schedule)

    def chunk_fp8(schedule="tile", out=out, metrics=metrics, metric_schedule="tile"):
        ops.paged_attention_kvc_chunk(out, q, kc8, vc8, HKV, scale, bt, lens, pos, qsl, qpos, buf, BS, ctx, nq,
                                      metrics=metrics, use_l2=True, kv_cache_dtype=kvd, k_scale=1.0, v_scale=1.0,
                                      schedule=schedule, metric_schedule=metric_schedule)

    if metric_leg:
        # the two metric passes behind the same output pass, and that pass alone
        sched = chunk_fp8 if fp8 else chunk
        rows = nq * (HQ // HKV)
        name = "wide" if rows > 32 else "short"
        legs = [m for m in ("tile", "rows") if metric_leg in (m, "both")]
        fns = [lambda: sched(name, metrics=None)] + [lambda m=m: sched(name, metric_schedule=m) for m in legs]
        (n_ms, n_lo, n_hi), *rest = timed_alternating(*fns, warmup=5, reps=40, batch=4)
        kbytes = S * HKV * ctx * HD * (1 if fp8 else 2)
        r = dict(layout=kvc.block_layout(), heads=[HQ, HKV], kv_cache_dtype=kvd, batch=S, ctx=ctx, nq=nq, rows=rows,
                 schedule=name, no_metric_ms=n_ms, no_metric_ms_min=n_lo, no_metric_ms_max=n_hi, k_bytes=kbytes)
        added = {}
        for m, (c_ms, c_lo, c_hi) in zip(legs, rest):
            r.update({f"{m}_call_ms": c_ms, f"{m}_call_ms_min": c_lo, f"{m}_call_ms_max": c_hi, f"{m}_metric_ms": c_ms - n_ms,
                      f"{m}_metric_fraction_of_8TBps_on_K": kbytes / max((c_ms - n_ms) * 1e-3, 1e-12) / PEAK})
            added[m] = torch.zeros_like(metrics)
            sched(name, metrics=added[m], metric_schedule=m)
        if len(legs) == 2:
            r["tile_over_rows_metric"] = r["tile_metric_ms"] / max(r["rows_metric_ms"], 1e-9)
            r["rows_vs_tile_max_rel_diff"] = float(((added["rows"] - added["tile"]).abs() /
                                                    added["tile"].abs().clamp_min(1e-30)).max())
        return r

    # the decode baseline: step j sees context_lens - (nq - 1 - j) slots and has one query per sequence
    q4, out_d = q.view(S, nq, HQ, HD), torch.empty((S, HQ, HD), dtype=q.dtype, device=dev)
    step_lens = [(lens - (nq - 1 - j)).contiguous() for j in range(nq)]
    step_last = [torch.full((S,), ctx - nq + j, dtype=torch.int32, device=dev) for j in range(nq)]
    temp = torch.empty(pos.shape + (HQ // HKV,), dtype=torch.float32, device=dev)

    def decode():
        for j in range(nq):
            if with_metric:
                ops.paged_attention_kvc_fused_metrics(out_d, metrics, q4[:, j], dkc, dvc, HKV, scale, bt, step_lens[j], pos,
                                                      step_last[j], buf, BS, ctx, None, kvd, 1.0, 1.0, use_l2=True,
                                                      temp_metrics=temp)
            else:
                ops.paged_attention_kvc_v1(out_d, temp, q4[:, j], dkc, dvc, HKV, scale, bt, step_lens[j], pos,
                                           step_last[j], buf, BS, ctx, None, kvd, 1.0, 1.0, False)

    extra = {}
    tiles = (nq + TILE - 1) // TILE
    visible = sum(max(0, ctx - (nq - 1 - min(nq, TILE * (t + 1)) + 1)) for t in range(tiles))    # per head, over the query tiles
    if wide:
        # fp8: wide, tile and split over the fp8 cache, and the wide schedule over the 2-byte cache of the same geometry
        sched = chunk_fp8 if fp8 else chunk
        fns = [lambda: sched("wide"), lambda: sched("tile"), lambda: sched("split")] + ([lambda: chunk("wide")] if fp8 else [])
        (w_ms, w_lo, w_hi), (t_ms, t_lo, t_hi), (s_ms, s_lo, s_hi), *rest = timed_alternating(*fns, warmup=5, reps=40, batch=4)
        o_w, o_t = torch.empty_like(q), torch.empty_like(q)
        sched("wide", o_w)
        sched("tile", o_t)
        byts = S * HKV * ctx * 2 * HD * (1 if fp8 else 2)
        if fp8:
            (a_ms, a_lo, a_hi), = rest
            extra = dict(kv_cache_dtype=kvd, wide_auto_ms=a_ms, wide_auto_ms_min=a_lo, wide_auto_ms_max=a_hi,
                         fp8_wide_over_auto_wide=w_ms / a_ms)
        return dict(layout=kvc.block_layout(), heads=[HQ, HKV], batch=S, ctx=ctx, nq=nq, metrics=with_metric, **extra,
                    wide_ms=w_ms, wide_ms_min=w_lo, wide_ms_max=w_hi, tile_ms=t_ms, tile_ms_min=t_lo, tile_ms_max=t_hi,
                    split_ms=s_ms, split_ms_min=s_lo, split_ms_max=s_hi, tile_over_wide=t_ms / w_ms,
                    split_over_wide=s_ms / w_ms, call_algorithmic_bytes=byts,
                    wide_fraction_of_8TBps=byts / (w_ms * 1e-3) / PEAK, tile_fraction_of_8TBps=byts / (t_ms * 1e-3) / PEAK,
                    split_fraction_of_8TBps=byts / (s_ms * 1e-3) / PEAK,
                    wide_vs_tile_max_abs_diff=float((o_w.float() - o_t.float()).abs().max()), out_tolerance=2e-3)
    if split:
        # the split schedule against the tile one (more than 32 rows per KV head: the short schedule does not apply)
        sched = chunk_fp8 if fp8 else chunk
        (s_ms, s_lo, s_hi), (t_ms, t_lo, t_hi) = timed_alternating(lambda: sched("split"), lambda: sched("tile"), warmup=5,
                                                                   reps=40, batch=4)
        o_s, o_t = torch.empty_like(q), torch.empty_like(q)
        sched("split", o_s)
        sched("tile", o_t)
        byts = S * HKV * visible * 2 * HD * (1 if fp8 else 2)
        pl = _lib.load().kvc_paged_attention_chunk_split_partition(ctx, nq)
        return dict(layout=kvc.block_layout(), kv_cache_dtype=kvd, batch=S, ctx=ctx, nq=nq, metrics=with_metric,
                    partition_len=pl, partitions=-(-ctx // pl), split_ms=s_ms, split_ms_min=s_lo, split_ms_max=s_hi,
                    tile_ms=t_ms, tile_ms_min=t_lo, tile_ms_max=t_hi, tile_over_split=t_ms / s_ms,
                    tile_algorithmic_bytes=byts, split_fraction_of_8TBps=byts / (s_ms * 1e-3) / PEAK,
                    tile_fraction_of_8TBps=byts / (t_ms * 1e-3) / PEAK,
                    split_vs_tile_max_abs_diff=float((o_s.float() - o_t.float()).abs().max()), out_tolerance=2e-3)
    if short:
        # fp8: short and tile over the fp8 cache, and the short schedule over the 2-byte cache of the same geometry
        sched = chunk_fp8 if fp8 else chunk
        fns = [lambda: sched("short"), lambda: sched("tile")] + ([lambda: chunk("short")] if fp8 else [])
        (s_ms, s_lo, s_hi), (t_ms, t_lo, t_hi), *rest = timed_alternating(*fns, warmup=5, reps=40)
        d_ms, d_lo, d_hi = timed(decode, 1, 5)
        o_s, o_t = torch.empty_like(q), torch.empty_like(q)
        sched("short", o_s)
        sched("tile", o_t)
        byts = S * HKV * ctx * 2 * HD * (1 if fp8 else 2)
        if fp8:
            (a_ms, a_lo, a_hi), = rest
            extra = dict(kv_cache_dtype=kvd, short_auto_ms=a_ms, short_auto_ms_min=a_lo, short_auto_ms_max=a_hi,
                         fp8_short_over_auto_short=s_ms / a_ms)
        return dict(layout=kvc.block_layout(), batch=S, ctx=ctx, nq=nq, metrics=with_metric, short_ms=s_ms, short_ms_min=s_lo,
                    short_ms_max=s_hi, tile_ms=t_ms, tile_ms_min=t_lo, tile_ms_max=t_hi, decode_x_nq_ms=d_ms,
                    decode_x_nq_ms_min=d_lo, decode_x_nq_ms_max=d_hi, tile_over_short=t_ms / s_ms,
                    decode_over_short=d_ms / s_ms, call_algorithmic_bytes=byts,
                    short_fraction_of_8TBps=byts / (s_ms * 1e-3) / PEAK, tile_fraction_of_8TBps=byts / (t_ms * 1e-3) / PEAK,
                    short_vs_tile_max_abs_diff=float((o_s.float() - o_t.float()).abs().max()), out_tolerance=2e-3, **extra)
    if fp8:
        (c_ms, c_lo, c_hi), (a_ms, a_lo, a_hi) = timed_alternating(chunk_fp8, chunk, warmup=3, reps=20)
        extra = dict(kv_cache_dtype=kvd, chunk_auto_ms=a_ms, chunk_auto_ms_min=a_lo, chunk_auto_ms_max=a_hi,
                     fp8_over_auto=c_ms / a_ms)
    else:
        c_ms, c_lo, c_hi = timed(chunk, 3, 20)
    d_ms, d_lo, d_hi = timed(decode, 1, 5)
    byts = S * HKV * visible * 2 * HD * (1 if fp8 else 2)
    return dict(layout=kvc.block_layout(), batch=S, ctx=ctx, nq=nq, metrics=with_metric, chunk_ms=c_ms, chunk_ms_min=c_lo,
                chunk_ms_max=c_hi, decode_x_nq_ms=d_ms, decode_x_nq_ms_min=d_lo, decode_x_nq_ms_max=d_hi,
                speedup=d_ms / c_ms, chunk_algorithmic_bytes=byts, chunk_fraction_of_8TBps=byts / (c_ms * 1e-3) / PEAK,
                **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="ctx,nq: a single configuration")
    ap.add_argument("--kv-cache-dtype", default="auto", choices=("auto", "fp8_e4m3", "fp8_e5m2"))
    ap.add_argument("--nq", default=None, help="1,2,4,8: the short schedule against the tile one; 16,32,64,128 (more than 32 rows per "
                    "KV head throughout): the split schedule against the tile one")
    ap.add_argument("--heads", default="8b", choices=("8b", "70b"), help="Llama-3-8B (32 / 8) or Llama-3-70B (64 / 8) heads")
    ap.add_argument("--wide", action="store_true", help="with --nq (33 .. 64 rows per KV head): wide against tile and split")
    ap.add_argument("--metric-schedule", default=None, choices=("tile", "rows", "both"),
                    help="with --nq (at most 64 rows per KV head): the metric passes behind one output schedule")
    ap.add_argument("--tree", action="store_true", help="with --nq (at most 64 rows per KV head, e.g. 7,15): one tree call "
                    "against the chain call of the same shape and against one chain call per root-to-leaf path")
    args = ap.parse_args()
    global S, HQ
    HQ = 64 if args.heads == "70b" else 32
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention_chunk: needs a GPU (nothing is estimated)")
    dev = "cuda:0"
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    cfgs = [(c, n) for c in (4096, 32768) for n in (16, 64, 256)]
    short = split = False
    if args.nq is not None:
        cfgs = [(c, int(n)) for c in (4096, 32768) for n in args.nq.split(",")]
        # more than 32 rows per KV head in every configuration: the split schedule's leg, otherwise the short one's
        split = all(n * (HQ // HKV) > 32 for _, n in cfgs) and not args.wide and not args.tree
        short = not split and not args.wide and not args.tree
    if args.tree and (args.nq is None or not all(n * (HQ // HKV) <= 64 for _, n in cfgs)):
        raise SystemExit("bench_attention_chunk: --tree takes --nq with at most 64 rows per KV head")
    if args.wide and (args.nq is None or not all(32 < n * (HQ // HKV) <= 64 for _, n in cfgs)):
        raise SystemExit("bench_attention_chunk: --wide takes --nq with 33 .. 64 rows per KV head")
    if args.metric_schedule and (args.nq is None or not all(n * (HQ // HKV) <= 64 for _, n in cfgs)):
        raise SystemExit("bench_attention_chunk: --metric-schedule takes --nq with at most 64 rows per KV head")
    if args.only:
        cfgs = [tuple(int(v) for v in args.only.split(","))]
    res = []
    for ctx in sorted({c for c, _ in cfgs}):
        state = make_cache(ctx, dev, gen, args.kv_cache_dtype)
        for layout in ("reference", "slot_major"):
            kvc.set_block_layout(layout)          # (random values: the same buffers serve either layout)
            nqs = [n for c, n in cfgs if c == ctx]
            for nq in nqs:
                for with_metric in (True,) if args.metric_schedule else (False, True):
                    if (args.wide or args.tree) and with_metric and not args.metric_schedule and (
                            layout != "reference" or nq != nqs[0]):
                        continue                  # one row with the metric per context
                    if args.tree:
                        r = run_tree(ctx, nq, with_metric, state, dev, gen, args.kv_cache_dtype)
                        res.append(r)
                        print(json.dumps(r), flush=True)
                        continue
                    r = run(ctx, nq, with_metric, state, dev, gen, args.kv_cache_dtype, short, split, args.wide,
                            args.metric_schedule)
                    res.append(r)
                    print(json.dumps(r), flush=True)
        del state
    kvc.set_block_layout("reference")
    for batch in (1, 64) if (short or split or args.wide) and not args.only else ():
        S = batch
        state = make_cache(4096, dev, gen, args.kv_cache_dtype)
        r = run(4096, cfgs[0][1] if args.wide else 16 if split else 4, bool(args.metric_schedule), state, dev, gen,
                args.kv_cache_dtype, short, split, args.wide, args.metric_schedule)
        res.append(r)
        print(json.dumps(r), flush=True)
        del state
    if args.json:
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
