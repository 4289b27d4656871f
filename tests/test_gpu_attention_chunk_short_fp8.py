"""The short schedule of paged_attention_kvc_chunk over fp8 caches (schedule="short" with e4m3 / e5m2 bytes, both block
layouts) against the float64 restatement of tests/test_gpu_attention_chunk.py, which is handed float(fp8) * scale.
Geometry of tests/test_gpu_attention_chunk_short.py (contexts on the partition boundaries the library reports), data
and tolerances of tests/test_gpu_attention_chunk_fp8.py: the bytes convert exactly and the scales are applied in fp32,
so output atol = tol * max(1, v_scale), rtol = tol with tol 2e-3 (fp16) / 1.6e-2 (bf16); added metric rtol 4e-4 +
atol 1e-9."""
import ctypes

import numpy as np
import pytest

from tests.attn_helpers import make_state
from tests.test_gpu_attention_chunk import reference

OFF, ONE = (0.37, 1.9), (1.0, 1.0)         # (k_scale, v_scale): off the powers of two, and none
CASES = [  # Hq, Hkv, hd, bs, dtype, kind, layout, metric, scales, NQ per sequence
    (32, 8, 128, 16, "f16", "fp8_e4m3", "reference", "l2", OFF, (1, 2, 3, 8, 5, 0)),      # qpk 4, R = 32: two row tiles
    (32, 8, 128, 16, "bf16", "fp8_e5m2", "slot_major", "l2", OFF, (1, 2, 3, 8, 5, 0)),
    (16, 2, 128, 32, "bf16", "fp8_e4m3", "reference", "l1", ONE, (1, 2, 4, 3, 4, 0)),     # qpk 8, bs 32
    (8, 2, 64, 32, "f16", "fp8_e5m2", "slot_major", "l2", OFF, (1, 4, 2, 3, 4, 0)),       # R = 16: one row tile, hd 64
    (2, 2, 64, 32, "bf16", "fp8_e4m3", "reference", None, OFF, (1, 15, 16, 17, 32, 0)),   # qpk 1: 32 limits in a tile
    (16, 1, 64, 16, "f16", "fp8_e4m3", "slot_major", "l1", ONE, (1, 2, 2, 1, 2, 0)),      # qpk 16
    (20, 1, 128, 32, "f16", "fp8_e5m2", "reference", "l2", OFF, (1, 1, 1, 1, 1, 0)),      # qpk 20: heads span both tiles
    (8, 2, 128, 16, "f16", "fp8_e5m2", "slot_major", None, OFF, (1, 4, 2, 3, 4, 0)),      # R = 16 at hd 128
    (8, 2, 64, 16, "bf16", "fp8_e5m2", "reference", "l2", ONE, (1, 4, 2, 3, 4, 0)),       # hd 64 over 16-slot blocks
]
_STATES = {}


def state(Hq, Hkv, hd, bs, dt, kind, scales, NQ, single=False):
    """one call's inputs (fp8 bytes for the WHOLE cache: saturating cast of N(0, 1)) and its reference results, computed
    once per shape and never modified; single: every context within one partition (no combine kernel)"""
    import torch
    key = (Hq, Hkv, hd, bs, dt, kind, scales, NQ, single)
    if key not in _STATES:
        from vllm_kvcompress_amd import _lib
        part = _lib.load().kvc_paged_attention_chunk_short_partition
        PL = part(1)
        cmax = PL if single else 5 * PL + 7
        assert part(cmax) == PL and PL % bs == 0
        rng = np.random.default_rng([Hq, Hkv, hd, bs, int(dt == "f16"), int(kind == "fp8_e5m2"), int(single)])
        S = len(NQ)
        g, c, pos, _ = make_state(rng, S, Hq, Hkv, hd, bs, cmax, cmax, dtype=dt)
        CTX = [PL - 1, PL, PL + 1, 2 * PL - 1, 2 * PL, 2 * PL + 1, cmax, 100, 96]
        ctx = np.array(CTX, np.int32)[(np.arange(S * Hkv) * 4 + Hq) % len(CTX)].reshape(S, Hkv)     # ragged per head
        if NQ[2] >= 2:
            ctx[2, 0] = PL + 1         # token nq - 2 has limit PL: its row sees nothing of the second partition
        ctx[3, 0] = NQ[3]              # pure causal: every visible key is new
        ctx[4, -1] = NQ[4] // 2        # fewer slots than new tokens: the leading rows see nothing
        if single:
            ctx = np.where(ctx > PL, ctx % PL + 1, ctx).astype(np.int32)
        qsl = np.concatenate([[0], np.cumsum(NQ)]).astype(np.int32)
        NB = c["vc"].shape[0]
        tdt = torch.float16 if dt == "f16" else torch.bfloat16
        tf8 = torch.float8_e5m2 if kind == "fp8_e5m2" else torch.float8_e4m3fn
        q = torch.from_numpy(rng.standard_normal((int(qsl[-1]), Hq, hd)).astype(np.float32)).to(tdt)
        k8 = torch.from_numpy(rng.standard_normal((NB, hd // 16, bs, 16)).astype(np.float32)).to(tf8)
        v8 = torch.from_numpy(rng.standard_normal((NB, hd, bs)).astype(np.float32)).to(tf8)
        kd = k8.double().numpy() * scales[0]                          # [NB, hd/16, bs, 16] -> [NB, hd/8, bs, 8]
        kd = kd.transpose(0, 2, 1, 3).reshape(NB, bs, hd // 8, 8).transpose(0, 2, 1, 3)
        qpos = np.concatenate([np.sort(rng.integers(cmax // 2, 2 * cmax, n)) for n in NQ]).astype(np.int32)
        buf = rng.integers(0, 40, S).astype(np.int32)
        st = dict(g=g, ctx=ctx, pos=pos, qsl=qsl, q=q, k8=k8.view(torch.uint8), v8=v8.view(torch.uint8), qpos=qpos, buf=buf,
                  bs=bs, Hkv=Hkv, NQ=NQ, PL=PL, kind=kind, scales=scales, m0=rng.random(pos.shape).astype(np.float32))
        for l2 in (True, False):
            st[l2] = reference(q.double().numpy(), kd, v8.double().numpy() * scales[1], g["block_tables"], ctx, pos, qsl,
                               qpos, buf, float(g["scale"]), l2)
        _STATES[key] = st
    return _STATES[key]


def run_short(st, layout, metrics0, use_l2=True, sentinel=7.0, dispatcher=False):
    """schedule="short" of the Python op, or (dispatcher) the compiled op, which chooses for itself"""
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import torch_ops
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev, g = "cuda:0", st["g"]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q, kc, vc = st["q"].to(dev), st["k8"].to(dev), st["v8"].to(dev)
    out = torch.full_like(q, sentinel)
    met = None if metrics0 is None else torch.from_numpy(metrics0.copy()).to(dev)
    convert_block_layout(kc, vc, "reference", layout)
    kvc.set_block_layout(layout)
    args = (out, q, kc, vc, st["Hkv"], float(g["scale"]), i32(g["block_tables"]), i32(st["ctx"]), i32(st["pos"]),
            i32(st["qsl"]), i32(st["qpos"]), i32(st["buf"]), st["bs"], int(st["ctx"].max()), max(st["NQ"]), met, use_l2)
    try:
        if dispatcher:
            torch_ops.register()
            torch.ops._C.kvcompress_paged_attention_chunk_fp8(*args, st["kind"], *st["scales"])
        else:
            ops.paged_attention_kvc_chunk(*args, kv_cache_dtype=st["kind"], k_scale=st["scales"][0],
                                          v_scale=st["scales"][1], schedule="short")
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,hd,bs,dt,kind,layout,metric,scales,NQ,single",
                         [c + (False,) for c in CASES] + [CASES[0] + (True,), CASES[3] + (True,)])
def test_short_schedule_fp8_matches_float64(Hq, Hkv, hd, bs, dt, kind, layout, metric, scales, NQ, single):
    st = state(Hq, Hkv, hd, bs, dt, kind, scales, NQ, single)
    assert (int(st["ctx"].max()) <= st["PL"]) == single              # one partition: no combine kernel
    use_l2 = metric != "l1"
    ref_out, ref_add, ref_hit = st[use_l2]
    zeros = None if metric is None else np.zeros_like(st["m0"])
    out, added = run_short(st, layout, zeros, use_l2)
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol * max(1.0, scales[1]), rtol=tol)    # (a leftover sentinel 7.0 fails this too)
    rows = np.repeat(np.arange(len(NQ)), NQ) == 4
    assert (out[rows][:NQ[4] - NQ[4] // 2, -(Hq // Hkv):] == 0).all()  # rows that see nothing
    if metric is None:
        return
    print("max rel metric error", (np.abs(added - ref_add) / np.maximum(ref_add, 1e-30))[ref_hit].max())
    assert np.allclose(added, ref_add, rtol=4e-4, atol=1e-9)          # from zeros: the store holds the added amount
    # from random values: one fp32 add of that amount per reached slot, every other slot bit-identical
    _, got = run_short(st, layout, st["m0"], use_l2)
    assert np.array_equal(got[~ref_hit].view(np.int32), st["m0"][~ref_hit].view(np.int32))
    assert np.array_equal(got[ref_hit], (st["m0"] + added)[ref_hit])


@pytest.mark.gpu
def test_short_schedule_fp8_is_deterministic():
    """the same bits from run to run -- and from the dispatcher op, which takes the short schedule for an eligible call
    (the tile schedule sums in another order)"""
    st = state(*CASES[0][:6], CASES[0][8], CASES[0][9])
    (o1, m1), (o2, m2), (o3, m3) = (run_short(st, "reference", st["m0"], dispatcher=d) for d in (False, False, True))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))
    assert np.array_equal(o1, o3) and np.array_equal(m1.view(np.int32), m3.view(np.int32))


def test_short_schedule_fp8_rule_and_refusals():
    """the host side (no device needed): who is eligible, refusals before anything is launched"""
    from vllm_kvcompress_amd import _lib
    lib = _lib.load()
    ok = lib.kvc_paged_attention_chunk_short_fp8_eligible
    assert [ok(32, 8, 8, 1), ok(32, 8, 8, 2), ok(20, 1, 1, 1), ok(32, 8, 8, 0), ok(32, 8, 9, 1), ok(32, 8, 9, 2)] == [1, 1, 1, 0, 0, 0]
    ws = ctypes.create_string_buffer(lib.kvc_paged_attention_chunk_workspace_bytes(4, 8) + 16)

    def error(k_scale=1.0, v_scale=1.0, **kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 4, 8, 2, 128, 16
        p.max_query_len = p.max_context_len = 4
        p.kv_cache_dtype = 1
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_short_fp8(ctypes.byref(p), k_scale, v_scale, None, 0, None) == 1
        return lib.kvc_last_error().decode()

    assert "kvc_paged_attention_chunk_short" in error(kv_cache_dtype=0)
    for bad in (0.0, -1.0, float("nan")):
        assert "finite and > 0" in error(k_scale=bad) and "finite and > 0" in error(v_scale=bad)
    assert "36 rows" in error(max_query_len=9)
    assert "head size: 96" in error(head_size=96)
    addr = (ctypes.addressof(ws) + 15) & ~15                           # two partitions and no partial scratch
    assert "partial scratch" in error(max_context_len=1000, workspace=addr, workspace_bytes=len(ws) - 16)
