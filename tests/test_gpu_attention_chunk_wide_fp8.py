"""The wide schedule of paged_attention_kvc_chunk over fp8 caches (schedule="wide" with e4m3 / e5m2 bytes, both block
layouts, 33 .. 64 rows per KV head) against the float64 restatement of tests/test_gpu_attention_chunk.py, which is
handed float(fp8) * scale: states, data and tolerances of tests/test_gpu_attention_chunk_short_fp8.py -- output atol =
tol * max(1, v_scale), rtol = tol with tol 2e-3 (fp16) / 1.6e-2 (bf16); added metric rtol 4e-4 + atol 1e-9."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_attention_chunk_short_fp8 import CASES as SHORT_CASES
from tests.test_gpu_attention_chunk_short_fp8 import OFF, ONE, run_short, state

CASES = [  # Hq, Hkv, hd, bs, dtype, kind, layout, metric, scales, NQ per sequence
    (16, 2, 128, 16, "f16", "fp8_e4m3", "reference", "l2", OFF, (1, 5, 3, 8, 6, 0)),      # R = 64: four row tiles, V rows in two blocks
    (16, 2, 128, 16, "bf16", "fp8_e5m2", "slot_major", "l2", OFF, (1, 5, 3, 8, 6, 0)),
    (8, 2, 128, 32, "bf16", "fp8_e4m3", "slot_major", "l1", ONE, (1, 9, 4, 12, 10, 0)),   # R = 48: three row tiles, bs 32
    (12, 1, 64, 32, "f16", "fp8_e5m2", "reference", "l1", OFF, (1, 2, 4, 3, 4, 0)),       # qpk 12: a token's heads straddle tiles
    (2, 2, 64, 16, "bf16", "fp8_e4m3", "slot_major", None, OFF, (1, 33, 48, 49, 64, 0)),  # qpk 1: 64 different limits in a workgroup
    (40, 1, 128, 32, "f16", "fp8_e5m2", "reference", "l2", OFF, (1, 1, 1, 1, 1, 0)),      # qpk 40: one token spans three tiles
    (8, 1, 64, 16, "f16", "fp8_e4m3", "reference", None, ONE, (1, 5, 3, 8, 6, 0)),        # hd 64, four tiles, bs 16
]


def run_wide(st, layout, metrics0, use_l2=True, poison=False):
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import _lib
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev, g = "cuda:0", st["g"]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q, kc, vc = st["q"].to(dev), st["k8"].to(dev), st["v8"].to(dev)
    out = torch.full_like(q, 7.0)                                        # (a leftover sentinel fails every comparison)
    met = None if metrics0 is None else torch.from_numpy(metrics0.copy()).to(dev)
    convert_block_layout(kc, vc, "reference", layout)
    if poison:                                                           # partials nobody wrote are NaN
        nbytes = _lib.load().kvc_paged_attention_chunk_short_workspace_bytes(len(st["NQ"]), q.shape[1], q.shape[2],
                                                                             max(st["NQ"]), int(st["ctx"].max()))
        ops.workspace(torch.device(dev), nbytes + 256, "attn_chunk_short").fill_(0xFF)
    kvc.set_block_layout(layout)
    try:
        ops.paged_attention_kvc_chunk(out, q, kc, vc, st["Hkv"], float(g["scale"]), i32(g["block_tables"]), i32(st["ctx"]),
                                      i32(st["pos"]), i32(st["qsl"]), i32(st["qpos"]), i32(st["buf"]), st["bs"],
                                      int(st["ctx"].max()), max(st["NQ"]), metrics=met, use_l2=use_l2,
                                      kv_cache_dtype=st["kind"], k_scale=st["scales"][0], v_scale=st["scales"][1],
                                      schedule="wide")
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


def check(st, case, out, added, second):
    """out and the metric added from zeros against float64; second: the metrics of a run that started from st["m0"]"""
    Hq, Hkv, _, _, dt, _, _, metric, scales, NQ = case
    ref_out, ref_add, ref_hit = st[metric != "l1"]
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol * max(1.0, scales[1]), rtol=tol)    # (a leftover sentinel 7.0 fails this too)
    rows = np.repeat(np.arange(len(NQ)), NQ) == 4
    assert (out[rows][:NQ[4] - NQ[4] // 2, -(Hq // Hkv):] == 0).all()  # rows that see nothing: exactly 0
    if metric is None:
        return
    print("max rel metric error", (np.abs(added - ref_add) / np.maximum(ref_add, 1e-30))[ref_hit].max())
    assert np.allclose(added, ref_add, rtol=4e-4, atol=1e-9)          # from zeros: the store holds the added amount
    # from random values: one fp32 add of that amount per reached slot, every other slot bit-identical
    assert np.array_equal(second[~ref_hit].view(np.int32), st["m0"][~ref_hit].view(np.int32))
    assert np.array_equal(second[ref_hit], (st["m0"] + added)[ref_hit])


@pytest.mark.gpu
@pytest.mark.parametrize("case,single", [(c, False) for c in CASES] + [(CASES[0], True), (CASES[3], True)])
def test_wide_schedule_fp8_matches_float64(case, single):
    Hq, Hkv, hd, bs, dt, kind, layout, metric, scales, NQ = case
    st = state(Hq, Hkv, hd, bs, dt, kind, scales, NQ, single)
    assert 32 < max(NQ) * (Hq // Hkv) <= 64
    assert (int(st["ctx"].max()) <= st["PL"]) == single              # one partition: no combine kernel
    use_l2 = metric != "l1"
    out, added = run_wide(st, layout, None if metric is None else np.zeros_like(st["m0"]), use_l2)
    second = None if metric is None else run_wide(st, layout, st["m0"], use_l2)[1]
    check(st, case, out, added, second)


@pytest.mark.gpu
def test_wide_schedule_fp8_reads_only_the_partials_it_wrote():
    """the partial scratch starts as NaN bytes: two runs give the same bits, and they still match float64"""
    case = CASES[0]
    st = state(*case[:6], case[8], case[9])
    (o1, m1), (o2, m2) = (run_wide(st, case[6], st["m0"], poison=True) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))
    out, added = run_wide(st, case[6], np.zeros_like(st["m0"]), poison=True)
    assert np.array_equal(out, o1)
    check(st, case, out, added, m1)


@pytest.mark.gpu
def test_wide_schedule_fp8_up_to_32_rows_is_the_short_schedule():
    case = SHORT_CASES[0]
    st = state(*case[:6], case[8], case[9])
    (o1, m1), (o2, m2) = run_wide(st, case[6], st["m0"]), run_short(st, case[6], st["m0"])
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


def test_wide_schedule_fp8_rule_and_refusals():
    """the host side (no device needed): who is eligible, refusals before anything is launched"""
    from vllm_kvcompress_amd import _lib
    lib = _lib.load()
    ok = lib.kvc_paged_attention_chunk_wide_fp8_eligible
    assert [ok(64, 8, 8, 1), ok(64, 8, 8, 2), ok(32, 8, 16, 1), ok(64, 8, 8, 0), ok(64, 8, 9, 1), ok(32, 8, 17, 2)] == [1, 1, 1, 0, 0, 0]
    ws = ctypes.create_string_buffer(lib.kvc_paged_attention_chunk_workspace_bytes(16, 8) + 16)
    addr = (ctypes.addressof(ws) + 15) & ~15

    def error(k_scale=1.0, v_scale=1.0, partial=None, partial_bytes=0, **kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 16, 8, 2, 128, 16
        p.max_query_len, p.max_context_len = 16, 16                    # 64 rows: the wide kernel's own checks
        p.kv_cache_dtype = 1
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_wide_fp8(ctypes.byref(p), k_scale, v_scale, partial, partial_bytes, None) == 1
        return lib.kvc_last_error().decode()

    assert "kvc_paged_attention_chunk_wide" in error(kv_cache_dtype=0)
    assert "data type of kv cache: 3" in error(kv_cache_dtype=3)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "finite and > 0" in error(k_scale=bad) and "finite and > 0" in error(v_scale=bad)
    msg = error(max_query_len=17)
    assert "68 rows" in msg and "64" in msg
    assert "head size: 96" in error(head_size=96)                      # the fp8 tile entry's refusals, behind the row check
    assert "head size: 96" in error(head_size=96, max_query_len=4)     # ... and through the short fp8 entry
    assert "ALiBi" in error(alibi_slopes=addr)
    two = dict(max_context_len=1000, workspace=addr, workspace_bytes=len(ws) - 16)   # two partitions
    need = lib.kvc_paged_attention_chunk_short_workspace_bytes(1, 8, 128, 16, 1000)
    part = ctypes.create_string_buffer(need + 32)
    paddr = (ctypes.addressof(part) + 15) & ~15
    assert "partial scratch" in error(**two)                           # missing
    assert "partial scratch" in error(partial=paddr, partial_bytes=need - 16, **two)        # too small
    assert "partial scratch" in error(partial=paddr + 8, partial_bytes=need, **two)          # misaligned
