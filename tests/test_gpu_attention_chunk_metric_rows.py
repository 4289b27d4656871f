"""The row-form metric pass of paged_attention_kvc_chunk (metric_schedule="rows": at most 64 (token, query head) rows
per KV head, kvc_paged_attention_chunk_metric_rows behind an output pass that ran without metrics) against the float64
restatement of tests/test_gpu_attention_chunk.py, on the states of the short and wide schedules' tests (2-byte and fp8
caches, contexts either side of 512-slot boundaries) and with the project's tolerance for the added metric, rtol 4e-4 +
atol 1e-9."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_attention_chunk_short as s2
from tests import test_gpu_attention_chunk_short_fp8 as s8
from tests import test_gpu_attention_chunk_wide as w2
from tests import test_gpu_attention_chunk_wide_fp8 as w8

# (case, single, schedule): 2-byte cases have 8 fields, fp8 cases 10; every case of the four lists that has a metric
_METRIC = [c for c in s2.CASES + w2.CASES + s8.CASES + w8.CASES if c[-2 if len(c) == 8 else -3] is not None]
RUNS = [(c, False, None) for c in _METRIC] + [(s2.CASES[0], True, None), (w8.CASES[0], True, None), (s2.CASES[3], False, "tile")]


def get_state(case, single=False):
    if len(case) == 8:
        return s2.short_state(*case[:5], case[7], single)
    return s8.state(*case[:6], case[8], case[9], single)


def run(case, st, metrics0, use_l2=True, schedule=None, metric_schedule="rows"):
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev, g, fp8 = "cuda:0", st["g"], len(case) == 10
    layout = case[6] if fp8 else case[5]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if fp8:
        q, kc, vc = st["q"].to(dev), st["k8"].to(dev), st["v8"].to(dev)
        kw = dict(kv_cache_dtype=st["kind"], k_scale=st["scales"][0], v_scale=st["scales"][1])
    else:
        tdt = torch.float16 if st["dt"] == "f16" else torch.bfloat16
        t = lambda bits: torch.from_numpy(np.ascontiguousarray(bits)).to(dev).view(tdt)
        q, kc, vc, kw = t(st["qbits"]), t(g["key_cache_bits"]), t(g["value_cache_bits"]), {}
    out = torch.full_like(q, 7.0)
    met = torch.from_numpy(metrics0.copy()).to(dev)
    convert_block_layout(kc, vc, "reference", layout)
    kvc.set_block_layout(layout)
    rows = max(st["NQ"]) * (case[0] // case[1])
    try:
        ops.paged_attention_kvc_chunk(out, q, kc, vc, st["Hkv"], float(g["scale"]), i32(g["block_tables"]), i32(st["ctx"]),
                                      i32(st["pos"]), i32(st["qsl"]), i32(st["qpos"]), i32(st["buf"]), st["bs"],
                                      int(st["ctx"].max()), max(st["NQ"]), metrics=met, use_l2=use_l2,
                                      schedule=schedule or ("short" if rows <= 32 else "wide"),
                                      metric_schedule=metric_schedule, **kw)
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), met.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case,single,schedule", RUNS)
def test_metric_rows_matches_float64(case, single, schedule):
    st = get_state(case, single)
    use_l2 = case[-2 if len(case) == 8 else -3] != "l1"
    _, ref_add, ref_hit = st[use_l2]
    _, added = run(case, st, np.zeros_like(st["m0"]), use_l2, schedule)
    print("max rel metric error", (np.abs(added - ref_add) / np.maximum(ref_add, 1e-30))[ref_hit].max())
    assert np.allclose(added, ref_add, rtol=4e-4, atol=1e-9)          # from zeros: the store holds the added amount
    # from random values: one fp32 add of that amount per reached slot, every other slot bit-identical
    _, got = run(case, st, st["m0"], use_l2, schedule)
    assert np.array_equal(got[~ref_hit].view(np.int32), st["m0"][~ref_hit].view(np.int32))
    assert np.array_equal(got[ref_hit], (st["m0"] + added)[ref_hit])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [w2.CASES[0], s8.CASES[1]])
def test_metric_rows_is_deterministic_and_leaves_out_alone(case):
    st = get_state(case)
    (o1, m1), (o2, m2) = (run(case, st, st["m0"]) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))
    z = np.zeros_like(st["m0"])
    (o3, a3), (o4, a4) = run(case, st, z), run(case, st, z, metric_schedule="tile")
    assert np.array_equal(o1, o3) and np.array_equal(o3, o4)         # out: the output pass's bits, whoever adds the metric
    assert np.allclose(a3, a4, rtol=4e-4, atol=1e-9)


def test_metric_rows_host_side():
    """no device needed: the keyword's default and refusal, the C entry's refusals before anything is launched"""
    import inspect
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import _lib
    lib = _lib.load()
    assert inspect.signature(ops.paged_attention_kvc_chunk).parameters["metric_schedule"].default == "tile"
    with pytest.raises(RuntimeError, match="metric_schedule"):
        ops.paged_attention_kvc_chunk(*([None] * 15), metric_schedule="bogus")
    store = ctypes.create_string_buffer(64)

    def error(k_scale=1.0, **kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 4, 8, 2, 128, 16
        p.max_query_len = p.max_context_len = 4
        p.metrics = ctypes.addressof(store)
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_metric_rows(ctypes.byref(p), k_scale, None) == 1
        return lib.kvc_last_error().decode()

    msg = error(num_heads=10, max_query_len=13)                        # 5 query heads per KV head: 65 rows
    assert "65 rows" in msg and "64" in msg
    assert "metrics" in error(metrics=None)
    assert "head size: 96" in error(head_size=96)
    assert "k_scale" in error(k_scale=2.0)
    assert "finite and > 0" in error(k_scale=float("nan"), kv_cache_dtype=1)
    assert "data type of kv cache: 3" in error(kv_cache_dtype=3)
