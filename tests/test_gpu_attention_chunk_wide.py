"""The wide schedule of paged_attention_kvc_chunk (schedule="wide": the short schedule's key split for 33 .. 64 (token,
query head) rows per KV head, three or four row tiles, Q in the LDS) against the float64 restatement of
tests/test_gpu_attention_chunk.py, on the states of tests/test_gpu_attention_chunk_short.py (contexts on the partition
boundaries the library reports) and with the project's tolerances: output 2e-3 (fp16) / 1.6e-2 (bf16), added metric
rtol 4e-4 + atol 1e-9."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_attention_chunk_short import CASES as SHORT_CASES
from tests.test_gpu_attention_chunk_short import run_short, short_state

CASES = [  # Hq, Hkv, hd, bs, dtype, layout, metric, NQ per sequence
    (16, 2, 128, 16, "f16", "reference", "l2", (1, 5, 3, 8, 6, 0)),      # qpk 8, R = 64: four row tiles, ragged nq
    (16, 2, 128, 16, "f16", "slot_major", "l2", (1, 5, 3, 8, 6, 0)),
    (8, 2, 128, 32, "bf16", "slot_major", "l1", (1, 9, 4, 12, 10, 0)),   # qpk 4, R = 48: three row tiles, bs 32
    (12, 1, 64, 32, "bf16", "reference", "l1", (1, 2, 4, 3, 4, 0)),      # qpk 12, R = 48: a token's heads straddle tiles
    (2, 2, 64, 16, "f16", "slot_major", None, (1, 33, 48, 49, 64, 0)),   # qpk 1: 64 different limits in a workgroup
    (40, 1, 128, 16, "f16", "reference", "l2", (1, 1, 1, 1, 1, 0)),      # qpk 40: one token spans three tiles
]


def run_wide(st, layout, metrics0, use_l2=True, schedule="wide", poison=False):
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import _lib
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev, g = "cuda:0", st["g"]
    tdt = torch.float16 if st["dt"] == "f16" else torch.bfloat16
    t = lambda bits: torch.from_numpy(np.ascontiguousarray(bits)).to(dev).view(tdt)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q, kc, vc = t(st["qbits"]), t(g["key_cache_bits"]), t(g["value_cache_bits"])
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
                                      int(st["ctx"].max()), max(st["NQ"]), metrics=met, use_l2=use_l2, schedule=schedule)
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


def check(st, case, out, added, second):
    """out and the metric added from zeros against float64; second: the metrics of a run that started from st["m0"]"""
    Hq, Hkv, _, _, dt, _, metric, NQ = case
    ref_out, ref_add, ref_hit = st[metric != "l1"]
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol, rtol=tol)              # (a leftover sentinel 7.0 fails this too)
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
def test_wide_schedule_matches_float64(case, single):
    Hq, Hkv, hd, bs, dt, layout, metric, NQ = case
    st = short_state(Hq, Hkv, hd, bs, dt, NQ, single)
    assert 32 < max(NQ) * (Hq // Hkv) <= 64
    assert (int(st["ctx"].max()) <= st["PL"]) == single              # one partition: no combine kernel
    use_l2 = metric != "l1"
    out, added = run_wide(st, layout, None if metric is None else np.zeros_like(st["m0"]), use_l2)
    second = None if metric is None else run_wide(st, layout, st["m0"], use_l2)[1]
    check(st, case, out, added, second)


@pytest.mark.gpu
def test_wide_schedule_is_deterministic():
    st = short_state(*CASES[0][:5], CASES[0][7])
    (o1, m1), (o2, m2) = (run_wide(st, "reference", st["m0"]) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


@pytest.mark.gpu
def test_wide_schedule_reads_only_the_partials_it_wrote():
    st = short_state(*CASES[0][:5], CASES[0][7])
    out, added = run_wide(st, "reference", np.zeros_like(st["m0"]), poison=True)
    check(st, CASES[0], out, added, run_wide(st, "reference", st["m0"], poison=True)[1])


@pytest.mark.gpu
def test_wide_schedule_up_to_32_rows_is_the_short_schedule():
    case = SHORT_CASES[0]
    st = short_state(*case[:5], case[7])
    (o1, m1), (o2, m2) = run_wide(st, case[5], st["m0"]), run_short(st, case[5], st["m0"])
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


def test_wide_schedule_rule_and_refusals():
    """the host side (no device needed): who is eligible, refusals before anything is launched"""
    from vllm_kvcompress_amd import _lib
    lib = _lib.load()
    ok = lib.kvc_paged_attention_chunk_wide_eligible
    assert [ok(64, 8, 8, 0), ok(64, 8, 9, 0), ok(32, 8, 16, 0), ok(32, 8, 17, 0), ok(64, 8, 8, 1)] == [1, 0, 1, 0, 0]

    def error(**kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 4, 8, 2, 128, 16
        p.max_query_len = p.max_context_len = 4
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_wide(ctypes.byref(p), None, 0, None) == 1
        return lib.kvc_last_error().decode()

    msg = error(max_query_len=17)                                      # 68 rows
    assert "rows" in msg and "64" in msg
    assert "fp8" in error(kv_cache_dtype=1)
    assert "head size: 96" in error(head_size=96)                      # F5's own refusals still run (through the short entry)
    assert "head size: 96" in error(head_size=96, max_query_len=16)    # ... and behind the wide kernel's own row check
