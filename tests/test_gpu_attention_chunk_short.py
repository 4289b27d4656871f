"""The short schedule of paged_attention_kvc_chunk (schedule="short": at most 32 (token, query head) rows per KV head,
the keys split over partitions of PL slots and merged by a second kernel) against the float64 restatement of
tests/test_gpu_attention_chunk.py, with that file's tolerances: output 2e-3 (fp16) / 1.6e-2 (bf16), added metric
rtol 4e-4 + atol 1e-9.  Contexts sit on the partition boundaries the library reports."""
import ctypes

import numpy as np
import pytest

from tests.attn_helpers import bf16_bits_to_f32, f32_to_bf16_bits, make_state
from tests.test_gpu_attention_chunk import reference

CASES = [  # Hq, Hkv, hd, bs, dtype, layout, metric, NQ per sequence
    (32, 8, 128, 16, "f16", "reference", "l2", (1, 2, 3, 8, 5, 0)),      # qpk 4, R = 32: two row tiles, ragged nq
    (32, 8, 128, 16, "f16", "slot_major", "l2", (1, 2, 3, 8, 5, 0)),
    (16, 2, 128, 16, "bf16", "reference", "l1", (1, 2, 4, 3, 4, 0)),     # qpk 8
    (8, 2, 64, 32, "f16", "slot_major", "l2", (1, 4, 2, 3, 4, 0)),       # R = 16: one row tile, hd 64, bs 32
    (2, 2, 64, 32, "bf16", "reference", None, (1, 15, 16, 17, 32, 0)),   # qpk 1: rows are tokens, 32 limits in a tile
    (16, 1, 64, 16, "f16", "slot_major", "l1", (1, 2, 2, 1, 2, 0)),      # qpk 16
    (20, 1, 128, 32, "bf16", "reference", "l2", (1, 1, 1, 1, 1, 0)),     # qpk 20: one token's heads span both tiles
]
_STATES = {}


def short_state(Hq, Hkv, hd, bs, dt, NQ, single=False):
    """one call's inputs and its reference results (computed once per shape, never modified); single: every context
    within one partition (the kernel writes out itself, no combine)"""
    key = (Hq, Hkv, hd, bs, dt, NQ, single)
    if key not in _STATES:
        from vllm_kvcompress_amd import _lib
        part = _lib.load().kvc_paged_attention_chunk_short_partition
        PL = part(1)
        cmax = PL if single else 5 * PL + 7
        assert part(cmax) == PL and PL % bs == 0
        rng = np.random.default_rng([Hq, Hkv, hd, bs, int(dt == "f16"), int(single)])
        S = len(NQ)
        g, c, pos, last = make_state(rng, S, Hq, Hkv, hd, bs, cmax, cmax, dtype=dt)
        # either side of one and two partitions, long, inside a block, on a block boundary -- ragged per head
        CTX = [PL - 1, PL, PL + 1, 2 * PL - 1, 2 * PL, 2 * PL + 1, cmax, 100, 96]
        ctx = np.array(CTX, np.int32)[(np.arange(S * Hkv) * 4 + Hq) % len(CTX)].reshape(S, Hkv)
        if NQ[2] >= 2:
            ctx[2, 0] = PL + 1         # token nq - 2 has limit PL: its row sees nothing of the second partition
        ctx[3, 0] = NQ[3]              # pure causal: every visible key is new
        ctx[4, -1] = NQ[4] // 2        # fewer slots than new tokens: the leading rows see nothing
        if single:
            ctx = np.where(ctx > PL, ctx % PL + 1, ctx).astype(np.int32)
        qsl = np.concatenate([[0], np.cumsum(NQ)]).astype(np.int32)
        qf = rng.standard_normal((int(qsl[-1]), Hq, hd)).astype(np.float32)
        qbits = qf.astype(np.float16).view(np.int16) if dt == "f16" else f32_to_bf16_bits(qf)
        qv = qbits.view(np.float16) if dt == "f16" else bf16_bits_to_f32(qbits)
        qpos = np.concatenate([np.sort(rng.integers(cmax // 2, 2 * cmax, n)) for n in NQ]).astype(np.int32)
        buf = rng.integers(0, 40, S).astype(np.int32)
        st = dict(g=g, ctx=ctx, pos=pos, qsl=qsl, qbits=qbits, qpos=qpos, buf=buf, bs=bs, dt=dt, Hkv=Hkv, NQ=NQ, PL=PL,
                  m0=rng.random(pos.shape).astype(np.float32))
        for l2 in (True, False):
            st[l2] = reference(qv, c["kc"], c["vc"], g["block_tables"], ctx, pos, qsl, qpos, buf, float(g["scale"]), l2)
        _STATES[key] = st
    return _STATES[key]


def run_short(st, layout, metrics0, use_l2=True, sentinel=7.0):
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
                                      int(st["ctx"].max()), max(st["NQ"]), metrics=met, use_l2=use_l2, schedule="short")
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("Hq,Hkv,hd,bs,dt,layout,metric,NQ,single",
                         [c + (False,) for c in CASES] + [CASES[0] + (True,), CASES[3] + (True,)])
def test_short_schedule_matches_float64(Hq, Hkv, hd, bs, dt, layout, metric, NQ, single):
    st = short_state(Hq, Hkv, hd, bs, dt, NQ, single)
    assert (int(st["ctx"].max()) <= st["PL"]) == single              # one partition: no combine kernel
    use_l2 = metric != "l1"
    ref_out, ref_add, ref_hit = st[use_l2]
    zeros = None if metric is None else np.zeros_like(st["m0"])
    out, added = run_short(st, layout, zeros, use_l2)
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol, rtol=tol)              # (a leftover sentinel 7.0 fails this too)
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
def test_short_schedule_is_deterministic():
    st = short_state(*CASES[0][:5], CASES[0][7])
    (o1, m1), (o2, m2) = (run_short(st, "reference", st["m0"]) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


def test_short_schedule_rule_and_refusals():
    """the host side (no device needed): who is eligible, the partition length, refusals before anything is launched"""
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import _lib
    lib = _lib.load()
    ok = lib.kvc_paged_attention_chunk_short_eligible
    assert [ok(32, 8, 8, 0), ok(32, 8, 9, 0), ok(20, 1, 1, 0), ok(20, 1, 2, 0)] == [1, 0, 1, 0]
    assert ok(32, 8, 4, 1) == 0 and ok(32, 8, 4, 2) == 0               # fp8 caches stay on the tile schedule
    for n in (1, 512, 513, 4096, 32768, 1 << 20):
        pl = lib.kvc_paged_attention_chunk_short_partition(n)
        assert pl > 0 and pl % 128 == 0
        nparts = -(-n // pl)
        assert lib.kvc_paged_attention_chunk_short_workspace_bytes(3, 32, 128, 8, n) == (
            0 if nparts == 1 else 3 * nparts * 8 * 32 * 130 * 4)

    def error(**kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 4, 8, 2, 128, 16
        p.max_query_len = p.max_context_len = 4
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_short(ctypes.byref(p), None, 0, None) == 1
        return lib.kvc_last_error().decode()

    assert "rows" in error(max_query_len=9)
    assert "fp8" in error(kv_cache_dtype=1)
    assert "head size: 96" in error(head_size=96)                      # F5's own refusals still run
    with pytest.raises(RuntimeError, match="schedule"):
        ops.paged_attention_kvc_chunk(*([None] * 15), schedule="bogus")
