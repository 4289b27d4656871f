"""The split schedule of paged_attention_kvc_chunk (schedule="split": the tile schedule's workgroups over key partitions
of PL slots, merged by a second kernel) over 2-byte and fp8 caches, against the float64 restatement of
tests/test_gpu_attention_chunk.py (fp8: handed float(fp8) * scale, as tests/test_gpu_attention_chunk_fp8.py does), with
the project's tolerances: output atol = tol * max(1, v_scale), rtol = tol, tol 2e-3 (fp16) / 1.6e-2 (bf16); added metric
rtol 4e-4 + atol 1e-9.  PL comes from the library, the contexts sit on its boundaries."""
import ctypes

import numpy as np
import pytest

from tests.attn_helpers import make_state
from tests.test_gpu_attention_chunk import reference

NQ, MAXQ = (16, 17, 40, 1, 9, 0), 40
OFF, ONE = (0.37, 1.9), (1.0, 1.0)         # (k_scale, v_scale): off the powers of two, and none
CASES = [  # Hq, Hkv, hd, bs, dtype, cache kind, scales, layout, metric
    (32, 8, 128, 16, "f16", "auto", ONE, "reference", "l2"),             # qpk 4: one head per wave (NT 1)
    (32, 8, 128, 16, "f16", "auto", ONE, "slot_major", "l2"),
    (16, 2, 128, 16, "bf16", "auto", ONE, "reference", "l1"),            # qpk 8 (NT 2)
    (2, 2, 64, 32, "f16", "auto", ONE, "slot_major", None),              # qpk 1: three idle waves
    (20, 1, 128, 16, "f16", "auto", ONE, "reference", "l2"),             # qpk 20: head groups of 16 (NT 4) and 4 (NT 1)
    (32, 8, 128, 16, "f16", "fp8_e4m3", OFF, "reference", "l2"),
    (16, 4, 64, 32, "bf16", "fp8_e5m2", ONE, "slot_major", "l2"),        # hd 64: waves 0, 1 fetch K, waves 2, 3 V
]
_STATES = {}


def state(Hq, Hkv, hd, bs, dt, kind, scales, single=False):
    """one call's inputs, made once per shape and never modified; single: every context within one partition"""
    import torch
    key = (Hq, Hkv, hd, bs, dt, kind, scales, single)
    if key in _STATES:
        return _STATES[key]
    from vllm_kvcompress_amd import _lib
    part = _lib.load().kvc_paged_attention_chunk_split_partition
    PL = part(1, MAXQ)
    cmax = 3 * PL + 7
    assert part(cmax, MAXQ) == PL and PL % bs == 0 and -(-cmax // PL) >= 2
    rng = np.random.default_rng([Hq, Hkv, hd, bs, int(dt == "f16"), len(kind), int(single)])
    S = len(NQ)
    g, c, pos, _ = make_state(rng, S, Hq, Hkv, hd, bs, cmax, cmax, dtype=dt)
    CTX = [PL - 1, PL, PL + 1, 2 * PL - 1, 2 * PL, 2 * PL + 1, cmax, 100, 96]
    ctx = np.array(CTX, np.int32)[(np.arange(S * Hkv) * 4 + Hq) % len(CTX)].reshape(S, Hkv)         # ragged per head
    ctx[0, 0] = PL + 5             # the limits of one tile (PL - 10 .. PL + 5) straddle the boundary
    ctx[1, 0] = NQ[1]              # pure causal: every visible key is new
    ctx[2, 0] = 2 * PL + 24        # tile 0 ends at limit 2 PL, tile 1 starts at 2 PL + 1: in the next partition
    ctx[3, -1] = cmax
    ctx[4, -1] = NQ[4] // 2        # fewer slots than new tokens: the leading rows see nothing
    if single:
        ctx = np.where(ctx > PL, ctx % PL + 1, ctx).astype(np.int32)
    qsl = np.concatenate([[0], np.cumsum(NQ)]).astype(np.int32)
    tdt = torch.float16 if dt == "f16" else torch.bfloat16
    q = torch.from_numpy(rng.standard_normal((int(qsl[-1]), Hq, hd)).astype(np.float32)).to(tdt)
    if kind == "auto":
        kc, vc = (torch.from_numpy(g[n]).view(tdt) for n in ("key_cache_bits", "value_cache_bits"))
        kd, vd = c["kc"], c["vc"]
    else:                          # fp8 bytes for the WHOLE cache: saturating cast of N(0, 1)
        NB = c["vc"].shape[0]
        tf8 = torch.float8_e5m2 if kind == "fp8_e5m2" else torch.float8_e4m3fn
        k8 = torch.from_numpy(rng.standard_normal((NB, hd // 16, bs, 16)).astype(np.float32)).to(tf8)
        v8 = torch.from_numpy(rng.standard_normal((NB, hd, bs)).astype(np.float32)).to(tf8)
        kd = k8.double().numpy() * scales[0]                              # [NB, hd/16, bs, 16] -> [NB, hd/8, bs, 8]
        kd = kd.transpose(0, 2, 1, 3).reshape(NB, bs, hd // 8, 8).transpose(0, 2, 1, 3)
        vd = v8.double().numpy() * scales[1]
        kc, vc = k8.view(torch.uint8), v8.view(torch.uint8)
    qpos = np.concatenate([np.sort(rng.integers(cmax // 2, 2 * cmax, n)) for n in NQ]).astype(np.int32)
    st = dict(bt=g["block_tables"], scale=float(g["scale"]), ctx=ctx, pos=pos, qsl=qsl, q=q, kc=kc, vc=vc, kd=kd, vd=vd,
              qpos=qpos, buf=rng.integers(0, 40, S).astype(np.int32), bs=bs, Hkv=Hkv, PL=PL, kind=kind, scales=scales,
              maxc=PL if single else cmax, m0=rng.random(pos.shape).astype(np.float32))
    _STATES[key] = st
    return st


def run(st, layout, metrics0, use_l2=True, schedule="split", seq=None):
    """seq: that sequence alone, under the same max_context_len / max_query_len"""
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import _lib
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev = "cuda:0"
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sl = slice(None) if seq is None else slice(seq, seq + 1)
    t0, t1 = (0, int(st["qsl"][-1])) if seq is None else (int(st["qsl"][seq]), int(st["qsl"][seq + 1]))
    qsl = st["qsl"] if seq is None else np.array([0, t1 - t0], np.int32)
    q, kc, vc = st["q"][t0:t1].to(dev), st["kc"].to(dev), st["vc"].to(dev)
    out = torch.full_like(q, 7.0)                                        # (a leftover sentinel fails every comparison)
    met = None if metrics0 is None else torch.from_numpy(metrics0.copy()).to(dev)
    convert_block_layout(kc, vc, "reference", layout)
    nbytes = _lib.load().kvc_paged_attention_chunk_split_workspace_bytes(t1 - t0, q.shape[1], q.shape[2], MAXQ, st["maxc"])
    ops.workspace(torch.device(dev), nbytes + 256, "attn_chunk_split").fill_(0xFF)      # partials nobody wrote are NaN
    kvc.set_block_layout(layout)
    try:
        ops.paged_attention_kvc_chunk(out, q, kc, vc, st["Hkv"], st["scale"], i32(st["bt"][sl]), i32(st["ctx"][sl]),
                                      i32(st["pos"]), i32(qsl), i32(st["qpos"][t0:t1]), i32(st["buf"][sl]), st["bs"], st["maxc"], MAXQ, metrics=met,
                                      use_l2=use_l2, kv_cache_dtype=st["kind"], k_scale=st["scales"][0],
                                      v_scale=st["scales"][1], schedule=schedule)
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,hd,bs,dt,kind,scales,layout,metric", CASES)
def test_split_schedule_matches_float64(Hq, Hkv, hd, bs, dt, kind, scales, layout, metric):
    st = state(Hq, Hkv, hd, bs, dt, kind, scales)
    use_l2 = metric != "l1"
    ref_out, ref_add, ref_hit = reference(st["q"].double().numpy(), st["kd"], st["vd"], st["bt"], st["ctx"], st["pos"],
                                          st["qsl"], st["qpos"], st["buf"], st["scale"], use_l2)
    out, added = run(st, layout, None if metric is None else np.zeros_like(st["m0"]), use_l2)
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol * max(1.0, scales[1]), rtol=tol)
    rows = np.repeat(np.arange(len(NQ)), NQ) == 4
    assert (out[rows][:NQ[4] - NQ[4] // 2, -(Hq // Hkv):] == 0).all()    # rows that see nothing: exactly 0
    if metric is None:
        return
    print("max rel metric error", (np.abs(added - ref_add) / np.maximum(ref_add, 1e-30))[ref_hit].max())
    assert np.allclose(added, ref_add, rtol=4e-4, atol=1e-9)            # from zeros: the store holds the added amount
    # from random values: one fp32 add of that amount per reached slot, every other slot bit-identical
    _, got = run(st, layout, st["m0"], use_l2)
    assert np.array_equal(got[~ref_hit].view(np.int32), st["m0"][~ref_hit].view(np.int32))
    assert np.array_equal(got[ref_hit], (st["m0"] + added)[ref_hit])


@pytest.mark.gpu
def test_split_schedule_is_deterministic_and_batch_independent():
    st = state(*CASES[0][:7])
    (o1, m1), (o2, m2) = (run(st, "reference", st["m0"]) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))
    alone, _ = run(st, "reference", None, seq=2)                         # the same two maxima: the same partitions
    assert np.array_equal(alone, o1[st["qsl"][2]:st["qsl"][3]])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[0], CASES[6]])
def test_split_schedule_with_one_partition_is_the_tile_schedule(case):
    st = state(*case[:7], single=True)
    assert int(st["ctx"].max()) <= st["maxc"] == st["PL"]
    (o1, m1), (o2, m2) = (run(st, case[7], st["m0"], schedule=s) for s in ("split", "tile"))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


def test_split_schedule_rule_and_refusals():
    """the host side (no device needed): the partition rule, the scratch size, refusals before anything is launched"""
    from vllm_kvcompress_amd import _lib
    lib = _lib.load()
    part, nbytes = lib.kvc_paged_attention_chunk_split_partition, lib.kvc_paged_attention_chunk_split_workspace_bytes
    grid = [(c, n) for c in (1, 1000, 4096, 4097, 32768, 100000, 1 << 20) for n in (1, 16, 17, 40, 128, 600)]
    for c, n in grid:
        pl = part(c, n)
        assert pl > 0 and pl % 32 == 0
        assert -(-c // pl) * -(-n // 16) <= 32 or pl >= c
        assert all(part(c2, n2) >= pl for c2, n2 in grid if c2 >= c and n2 >= n)        # non-decreasing in either
        nparts = -(-c // pl)
        assert nbytes(77, 32, 128, n, c) == (0 if nparts == 1 else nparts * 77 * 32 * 130 * 4)
    ws = ctypes.create_string_buffer(lib.kvc_paged_attention_chunk_workspace_bytes(4, 8) + 16)

    def error(k_scale=1.0, v_scale=1.0, **kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 4, 8, 2, 128, 16
        p.max_query_len = p.max_context_len = 4
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_split(ctypes.byref(p), k_scale, v_scale, None, 0, None) == 1
        return lib.kvc_last_error().decode()

    addr = (ctypes.addressof(ws) + 15) & ~15                             # many partitions and no partial scratch
    assert "partial scratch" in error(max_context_len=1 << 20, workspace=addr, workspace_bytes=len(ws) - 16)
    assert "fp8 cache" in error(k_scale=0.5) and "fp8 cache" in error(v_scale=2.0)
    for bad in (float("inf"), float("nan"), 0.0):
        assert "finite and > 0" in error(k_scale=bad, kv_cache_dtype=1) and "finite and > 0" in error(v_scale=bad, kv_cache_dtype=2)
    assert "head size: 96" in error(head_size=96) and "head size: 96" in error(head_size=96, kv_cache_dtype=1)
