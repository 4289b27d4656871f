"""paged_attention_kvc_chunk over fp8 caches (e4m3 / e5m2, both block layouts) against the float64 restatement of
tests/test_gpu_attention_chunk.py, which is handed float(fp8) * scale.  The kernels convert the bytes exactly and
apply k_scale / v_scale in fp32, so the tolerances are the unquantised test's (output 2e-3 fp16 / 1.6e-2 bf16,
atol = rtol; added metric rtol 4e-4 + atol 1e-9) with the absolute part of the output times max(1, v_scale): the
output is linear in v_scale and the arithmetic is otherwise that of the "auto" path."""
import ctypes

import numpy as np
import pytest

from tests.attn_helpers import make_state
from tests.test_gpu_attention_chunk import CTX, CTX_MAX, NQ, reference

_STATES = {}


def fp8_state(Hq, Hkv, hd, bs, dt, kind, scales):
    """geometry of the unquantised chunk test, fp8 bytes for the WHOLE cache (saturating cast of N(0, 1): no NaN or inf
    byte anywhere) and the reference results; computed once per case, never modified"""
    import torch
    key = (Hq, Hkv, hd, bs, dt, kind, scales)
    if key not in _STATES:
        rng = np.random.default_rng([Hq, Hkv, hd, bs, int(dt == "f16"), int(kind == "fp8_e5m2")])
        S = len(NQ)
        g, c, pos, _ = make_state(rng, S, Hq, Hkv, hd, bs, CTX_MAX, CTX_MAX, dtype=dt)
        ctx = np.array(CTX, np.int32)[(np.arange(S * Hkv) * 3) % len(CTX)].reshape(S, Hkv)    # ragged per head
        ctx[3, 0] = NQ[3]              # pure causal: every visible key is new
        ctx[4, -1] = 20                # fewer slots than new tokens: the leading rows see nothing
        qsl = np.concatenate([[0], np.cumsum(NQ)]).astype(np.int32)
        NB, T = c["vc"].shape[0], int(qsl[-1])
        tdt = torch.float16 if dt == "f16" else torch.bfloat16
        tf8 = torch.float8_e5m2 if kind == "fp8_e5m2" else torch.float8_e4m3fn
        q = torch.from_numpy(rng.standard_normal((T, Hq, hd)).astype(np.float32)).to(tdt)
        k8 = torch.from_numpy(rng.standard_normal((NB, hd // 16, bs, 16)).astype(np.float32)).to(tf8)
        v8 = torch.from_numpy(rng.standard_normal((NB, hd, bs)).astype(np.float32)).to(tf8)
        kd = k8.double().numpy() * scales[0]                          # [NB, hd/16, bs, 16] -> [NB, hd/8, bs, 8]
        kd = kd.transpose(0, 2, 1, 3).reshape(NB, bs, hd // 8, 8).transpose(0, 2, 1, 3)
        vd = v8.double().numpy() * scales[1]
        qpos = np.concatenate([np.sort(rng.integers(CTX_MAX // 2, 2 * CTX_MAX, n)) for n in NQ]).astype(np.int32)
        buf = rng.integers(0, 40, S).astype(np.int32)
        st = dict(g=g, ctx=ctx, pos=pos, qsl=qsl, q=q, k8=k8.view(torch.uint8), v8=v8.view(torch.uint8), qpos=qpos,
                  buf=buf, bs=bs, Hkv=Hkv, kind=kind, scales=scales, m0=rng.random(pos.shape).astype(np.float32))
        for l2 in (True, False):
            st[l2] = reference(q.double().numpy(), kd, vd, g["block_tables"], ctx, pos, qsl, qpos, buf, float(g["scale"]), l2)
        _STATES[key] = st
    return _STATES[key]


def run_chunk(st, layout, metrics0, use_l2=True, sentinel=7.0):
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev, g = "cuda:0", st["g"]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q, kc, vc = st["q"].to(dev), st["k8"].to(dev), st["v8"].to(dev)
    out = torch.full_like(q, sentinel)
    met = None if metrics0 is None else torch.from_numpy(metrics0.copy()).to(dev)
    convert_block_layout(kc, vc, "reference", layout)
    kvc.set_block_layout(layout)
    try:
        ops.paged_attention_kvc_chunk(out, q, kc, vc, st["Hkv"], float(g["scale"]), i32(g["block_tables"]), i32(st["ctx"]),
                                      i32(st["pos"]), i32(st["qsl"]), i32(st["qpos"]), i32(st["buf"]), st["bs"],
                                      int(st["ctx"].max()), max(NQ), metrics=met, use_l2=use_l2,
                                      kv_cache_dtype=st["kind"], k_scale=st["scales"][0], v_scale=st["scales"][1])
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,hd,bs,dt,kind,layout,metric,scales", [
    (32, 8, 128, 16, "f16", "fp8_e4m3", "reference", "l2", (0.37, 1.9)),     # Llama-shaped; scales off the powers of two
    (8, 2, 128, 16, "f16", "fp8_e5m2", "slot_major", "l2", (0.5, 2.0)),       # qpk 4: one row tile per wave
    (16, 2, 128, 16, "bf16", "fp8_e4m3", "slot_major", "l1", (0.37, 1.9)),   # qpk 8: two row tiles per wave
    (2, 2, 64, 32, "f16", "fp8_e5m2", "reference", "l2", (1.0, 1.0)),        # qpk 1: one wave computes; K / V wave split
    (16, 2, 64, 32, "bf16", "fp8_e5m2", "slot_major", None, (0.37, 1.9)),
    (8, 2, 128, 32, "f16", "fp8", "slot_major", "l1", (1.0, 1.0)),
    (20, 1, 64, 16, "f16", "fp8_e4m3", "reference", "l2", (0.5, 2.0)),       # qpk 20: two head groups (16 + 4)
    (8, 2, 64, 16, "bf16", "fp8_e4m3", "slot_major", "l2", (1.3, 0.6)),
    (2, 2, 128, 16, "bf16", "fp8_e5m2", "reference", None, (0.5, 2.0)),
    (12, 1, 128, 32, "f16", "fp8_e4m3", "reference", "l2", (0.37, 1.9)),     # qpk 12: three row tiles per wave of four
])
def test_chunk_attention_fp8_matches_float64(Hq, Hkv, hd, bs, dt, kind, layout, metric, scales):
    st = fp8_state(Hq, Hkv, hd, bs, dt, kind, scales)
    use_l2 = metric != "l1"
    ref_out, ref_add, ref_hit = st[use_l2]
    zeros = None if metric is None else np.zeros_like(st["m0"])
    out, added = run_chunk(st, layout, zeros, use_l2)
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol * max(1.0, scales[1]), rtol=tol)    # (a leftover sentinel 7.0 fails this too)
    rows = np.repeat(np.arange(len(NQ)), NQ) == 4
    assert (out[rows][:NQ[4] - 20, -(Hq // Hkv):] == 0).all()         # rows that see nothing
    if metric is None:
        return
    print("max rel metric error", (np.abs(added - ref_add) / np.maximum(ref_add, 1e-30))[ref_hit].max())
    assert np.allclose(added, ref_add, rtol=4e-4, atol=1e-9)          # from zeros: the store holds the added amount
    # from random values: one fp32 add of that amount per reached slot, every other slot bit-identical
    _, got = run_chunk(st, layout, st["m0"], use_l2)
    assert np.array_equal(got[~ref_hit].view(np.int32), st["m0"][~ref_hit].view(np.int32))
    assert np.array_equal(got[ref_hit], (st["m0"] + added)[ref_hit])


@pytest.mark.gpu
def test_chunk_attention_fp8_is_deterministic():
    st = fp8_state(32, 8, 128, 16, "f16", "fp8_e4m3", (0.37, 1.9))
    (o1, m1), (o2, m2) = (run_chunk(st, "reference", st["m0"]) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


def test_chunk_attention_fp8_refusals_and_registration():
    """refused before anything is launched (no device needed), each with the reason in the message"""
    import torch
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import _lib, torch_ops
    lib = _lib.load()

    def error(k_scale=1.0, v_scale=1.0, **kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 4, 8, 2, 128, 16
        p.max_query_len = p.max_context_len = 4
        p.kv_cache_dtype = 1
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_fp8(ctypes.byref(p), k_scale, v_scale, None) == 1
        return lib.kvc_last_error().decode()

    assert "kvc_paged_attention_chunk" in error(kv_cache_dtype=0)
    for bad in (0.0, -1.0, float("nan")):
        assert "finite and > 0" in error(k_scale=bad) and "finite and > 0" in error(v_scale=bad)
    assert "ALiBi" in error(alibi_slopes=ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p))
    assert "head size: 96" in error(head_size=96)
    assert "block size: 8" in error(block_size=8)
    assert "cache blocks must be 16-byte aligned" in error(query=16, out=16, q_stride=1024, out_stride=1024, key_cache=24,
                                                            value_cache=32, kv_block_stride=2048)
    assert "cache blocks must be 16-byte aligned" in error(query=16, out=16, q_stride=1024, out_stride=1024, key_cache=32,
                                                            value_cache=32, kv_block_stride=2056)
    torch_ops.register()
    assert hasattr(torch.ops._C, "kvcompress_paged_attention_chunk_fp8")
    # the Python op, before anything else is looked at: a 2-byte cache under an fp8 name, scales without an fp8 cache
    q, i = torch.zeros((4, 8, 128), dtype=torch.float16), torch.zeros(4, dtype=torch.int32)
    args = (torch.zeros_like(q), q, torch.zeros((4, 16, 16, 8), dtype=torch.float16), torch.zeros((4, 128, 16), dtype=torch.float16),
            2, 1.0, i, i, i, i, i, i, 16, 4, 4)
    with pytest.raises(RuntimeError, match="1-byte"):
        ops.paged_attention_kvc_chunk(*args, kv_cache_dtype="fp8_e4m3")
    with pytest.raises(RuntimeError, match="belong to an fp8 cache"):
        ops.paged_attention_kvc_chunk(*args, k_scale=0.5)
