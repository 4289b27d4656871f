"""Query-block paged attention over the per-head cache with KV metrics (paged_attention_kvc_chunk) against a
plain float64 restatement.  The output pass works on query tiles of TILE = 16 tokens, the metric pass on key
partitions of 256 slots; tolerances are the decode tests' (tests/test_gpu_attention.py): output 2e-3 (fp16) /
1.6e-2 (bf16), the added metric rtol 4e-4 (twice the 2e-4 on p: squaring doubles a relative error) + atol 1e-9."""
import ctypes

import numpy as np
import pytest

from tests.attn_helpers import bf16_bits_to_f32, f32_to_bf16_bits, make_state

TILE = 16
NQ = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 0]                  # query tokens of the six sequences of a call
# contexts: inside a block, on a block boundary, either side of a 256- and a 512-slot partition boundary, long
CTX = [511, 512, 513, 1300, 255, 256, 257, 100, 96, 1290]
CTX_MAX = 1300


def reference(q, kc, vc, bt, ctx, pos, qsl, qpos, buf, scale, use_l2):
    """-> out [T, Hq, hd], added metric [NB, bs], reached slots [NB, bs]; float64, caches in the reference layout"""
    T, Hq, hd = q.shape
    NB, _, bs = vc.shape
    Hkv = ctx.shape[1]
    qpk = Hq // Hkv
    out, add, hit = np.zeros((T, Hq, hd)), np.zeros(NB * bs), np.zeros(NB * bs, bool)
    for s in range(len(qsl) - 1):
        q0, q1 = int(qsl[s]), int(qsl[s + 1])
        nq = q1 - q0
        for h in range(Hkv if nq else 0):
            n = int(ctx[s, h])
            blocks = bt[s, h, :(n + bs - 1) // bs]
            K = kc[blocks].transpose(0, 2, 1, 3).reshape(-1, hd)[:n].astype(np.float64)
            V = vc[blocks].transpose(0, 2, 1).reshape(-1, hd)[:n].astype(np.float64)
            slots = (blocks[:, None] * bs + np.arange(bs)).reshape(-1)[:n]
            vis = np.arange(n)[None, :] < np.maximum(0, n - (nq - 1 - np.arange(nq)))[:, None]
            win = vis & (pos.reshape(-1)[slots][None, :] <= (qpos[q0:q1] - buf[s])[:, None])
            hit[slots] |= win.any(0)
            for hq in range(h * qpk, (h + 1) * qpk):
                S = np.where(vis, scale * q[q0:q1, hq].astype(np.float64) @ K.T, -np.inf)
                mx = S.max(1, keepdims=True, initial=-np.inf)
                p = np.where(vis, np.exp(S - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
                p /= np.maximum(p.sum(1, keepdims=True), 1e-300)
                out[q0:q1, hq] = p @ V
                add[slots] += np.where(win, p * p if use_l2 else p, 0.0).sum(0)
    return out, add.reshape(NB, bs), hit.reshape(NB, bs)


_STATES = {}


def chunk_state(Hq, Hkv, hd, bs, dt):
    """one call's inputs and its reference results (computed once per shape, never modified)"""
    key = (Hq, Hkv, hd, bs, dt)
    if key not in _STATES:
        rng = np.random.default_rng([Hq, Hkv, hd, bs, int(dt == "f16")])
        S = len(NQ)
        g, c, pos, last = make_state(rng, S, Hq, Hkv, hd, bs, CTX_MAX, CTX_MAX, dtype=dt)
        ctx = np.array(CTX, np.int32)[(np.arange(S * Hkv) * 3) % len(CTX)].reshape(S, Hkv)    # ragged per head
        ctx[3, 0] = NQ[3]              # pure causal: every visible key is new
        ctx[4, -1] = 20                # fewer slots than new tokens: the leading rows see nothing
        assert (ctx[np.arange(S) != 4] >= np.array(NQ)[np.arange(S) != 4, None]).all()
        qsl = np.concatenate([[0], np.cumsum(NQ)]).astype(np.int32)
        T = int(qsl[-1])
        qf = rng.standard_normal((T, Hq, hd)).astype(np.float32)
        qbits = qf.astype(np.float16).view(np.int16) if dt == "f16" else f32_to_bf16_bits(qf)
        qv = qbits.view(np.float16) if dt == "f16" else bf16_bits_to_f32(qbits)
        qpos = np.concatenate([np.sort(rng.integers(CTX_MAX // 2, 2 * CTX_MAX, n)) for n in NQ]).astype(np.int32)
        buf = rng.integers(0, 40, S).astype(np.int32)
        st = dict(g=g, ctx=ctx, pos=pos, qsl=qsl, qbits=qbits, qpos=qpos, buf=buf, hd=hd, bs=bs, dt=dt, Hkv=Hkv,
                  m0=rng.random(pos.shape).astype(np.float32))
        for l2 in (True, False):
            st[l2] = reference(qv, c["kc"], c["vc"], g["block_tables"], ctx, pos, qsl, qpos, buf, float(g["scale"]), l2)
        _STATES[key] = st
    return _STATES[key]


def run_chunk(st, layout, metrics0, use_l2=True, sentinel=7.0):
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev, g = "cuda:0", st["g"]
    tdt = torch.float16 if st["dt"] == "f16" else torch.bfloat16
    t = lambda bits: torch.from_numpy(np.ascontiguousarray(bits)).to(dev).view(tdt)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q, kc, vc = t(st["qbits"]), t(g["key_cache_bits"]), t(g["value_cache_bits"])
    out = torch.full_like(q, sentinel)
    met = None if metrics0 is None else torch.from_numpy(metrics0.copy()).to(dev)
    convert_block_layout(kc, vc, "reference", layout)
    kvc.set_block_layout(layout)
    try:
        ops.paged_attention_kvc_chunk(out, q, kc, vc, st["Hkv"], float(g["scale"]), i32(g["block_tables"]), i32(st["ctx"]),
                                      i32(st["pos"]), i32(st["qsl"]), i32(st["qpos"]), i32(st["buf"]), st["bs"],
                                      int(st["ctx"].max()), max(NQ), metrics=met, use_l2=use_l2)
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,hd,bs,dt,layout,metric", [
    (32, 8, 128, 16, "f16", "reference", "l2"),          # Llama-shaped
    (32, 8, 128, 16, "f16", "slot_major", "l2"),
    (16, 2, 128, 16, "bf16", "reference", "l1"),         # qpk 8: two row tiles per wave
    (2, 2, 64, 32, "f16", "reference", "l2"),            # qpk 1: one wave computes
    (16, 2, 64, 32, "bf16", "slot_major", None),
    (8, 2, 128, 32, "f16", "slot_major", "l1"),
    (20, 1, 64, 16, "f16", "reference", "l2"),           # qpk 20: two head groups (16 + 4)
    (8, 2, 64, 16, "bf16", "slot_major", "l2"),
    (2, 2, 128, 16, "bf16", "reference", None),
    (12, 1, 128, 32, "f16", "reference", "l2"),          # qpk 12: three row tiles per wave of four
])
def test_chunk_attention_matches_float64(Hq, Hkv, hd, bs, dt, layout, metric):
    st = chunk_state(Hq, Hkv, hd, bs, dt)
    use_l2 = metric != "l1"
    ref_out, ref_add, ref_hit = st[use_l2]
    zeros = None if metric is None else np.zeros_like(st["m0"])
    out, added = run_chunk(st, layout, zeros, use_l2)
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol, rtol=tol)              # (a leftover sentinel 7.0 fails this too)
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
def test_chunk_attention_is_deterministic():
    st = chunk_state(32, 8, 128, 16, "f16")
    (o1, m1), (o2, m2) = (run_chunk(st, "reference", st["m0"]) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


def test_chunk_attention_refusals_and_registration():
    """refused before anything is launched (no device needed), each with the reason in the message"""
    import torch
    from vllm_kvcompress_amd import _lib, torch_ops
    lib = _lib.load()

    def error(**kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 4, 8, 2, 128, 16
        p.max_query_len = p.max_context_len = 4
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk(ctypes.byref(p), None) == 1
        return lib.kvc_last_error().decode()

    assert "fp8" in error(kv_cache_dtype=1)
    assert "ALiBi" in error(alibi_slopes=ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p))
    assert "head size: 96" in error(head_size=96)
    assert "block size: 8" in error(block_size=8)
    assert "multiple of num_kv_heads" in error(num_heads=9)
    assert "aligned" in error(query=8, out=16, q_stride=1024, out_stride=1024)
    assert lib.kvc_paged_attention_chunk_workspace_bytes(10, 32) == 10 * 32 * 8
    torch_ops.register()
    assert hasattr(torch.ops._C, "kvcompress_paged_attention_chunk")
