"""Draft-tree verification of paged_attention_kvc_chunk (tree_mask: one 64-bit word per query token) against a float64
function that applies the rule of include/kvc_mi355x.h literally.  States of the short / wide test files (contexts on
the partition boundaries the library reports, a head with fewer slots than new tokens, a pure-new-keys head) with their
tolerances: output 2e-3 (fp16) / 1.6e-2 (bf16), over fp8 caches atol * max(1, v_scale); added metric rtol 4e-4 + atol
1e-9."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_attention_chunk_short as s2
from tests import test_gpu_attention_chunk_short_fp8 as s8
from tests import test_gpu_attention_chunk_wide as w2
from tests import test_gpu_attention_chunk_wide_fp8 as w8
from tests.attn_helpers import bf16_bits_to_f32
from tests.test_gpu_attention_chunk_metric_rows import get_state

RUNS = [  # (case, single): 2-byte cases have 8 fields, fp8 cases 10
    (s2.CASES[0], False),   # R = 32: two row tiles, qpk 4, hd 128, bs 16, fp16, reference blocks, l2
    (s2.CASES[3], False),   # R = 16: one row tile, hd 64, bs 32, slot-major
    (s2.CASES[2], False),   # qpk 8, bf16, l1
    (s2.CASES[4], False),   # qpk 1: 32 words in a tile, no metric
    (s2.CASES[6], False),   # qpk 20: one token's heads straddle the two tiles
    (w2.CASES[0], False),   # R = 64: four row tiles, qpk 8
    (w2.CASES[2], False),   # R = 48: three row tiles, bf16, slot-major, bs 32, l1
    (w2.CASES[4], False),   # qpk 1, nq up to 64: every bit of a word
    (s8.CASES[0], False),   # e4m3, short kernel, reference blocks
    (w8.CASES[1], False),   # e5m2, wide kernel, slot-major, bf16
    (s2.CASES[0], True),    # one partition: no combine kernel
    (w2.CASES[3], True),    # ... wide, qpk 12: a token's heads straddle tiles
]
_REFS = {}


def forest(NQ, seed):
    """per token the word of a random forest: its parent's word (parent index < own index, or none) plus its own bit.
    Sequence 3, whose head 0 holds new slots only (base 0): token 1 sees nothing at all, and nobody sees its slot"""
    rng, words = np.random.default_rng(seed), []
    for s, nq in enumerate(NQ):
        w = []
        for j in range(nq):
            parent = int(rng.integers(-1, j))
            w.append((w[parent] if parent >= 0 else 0) | (1 << j))
        if s == 3 and nq >= 2:
            w = [0 if j == 1 else x & ~2 for j, x in enumerate(w)]
        words += w
    return np.array(words, np.uint64)


def tree_reference(q, kc, vc, bt, ctx, pos, qsl, qpos, buf, scale, use_l2, words):
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
            e = np.arange(n) - (n - nq)                                  # slot i has e = i - base
            bit = (words[q0:q1, None] >> np.clip(e, 0, 63).astype(np.uint64)[None, :]) & np.uint64(1)
            vis = (e < 0)[None, :] | ((e < nq)[None, :] & (bit != 0))
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


def tree_state(case, single):
    """the shared state of the case, its words and the tree reference (computed once, never modified)"""
    import torch
    key = (case, single)
    if key not in _REFS:
        st, fp8 = get_state(case, single), len(case) == 10
        g, words = st["g"], forest(st["NQ"], [*case[:4], int(single)])
        if fp8:
            tf8 = torch.float8_e5m2 if st["kind"] == "fp8_e5m2" else torch.float8_e4m3fn
            NB, hd, bs = st["v8"].shape
            kd = st["k8"].view(tf8).double().numpy() * st["scales"][0]   # [NB, hd/16, bs, 16] -> [NB, hd/8, bs, 8]
            kd = kd.transpose(0, 2, 1, 3).reshape(NB, bs, hd // 8, 8).transpose(0, 2, 1, 3)
            q, vd = st["q"].double().numpy(), st["v8"].view(tf8).double().numpy() * st["scales"][1]
        else:
            vals = (lambda b: b.view(np.float16)) if st["dt"] == "f16" else bf16_bits_to_f32
            q, kd, vd = vals(st["qbits"]), vals(g["key_cache_bits"]), vals(g["value_cache_bits"])
        use_l2 = case[-2 if len(case) == 8 else -3] != "l1"
        _REFS[key] = st, words, tree_reference(q, kd, vd, g["block_tables"], st["ctx"], st["pos"], st["qsl"], st["qpos"],
                                               st["buf"], float(g["scale"]), use_l2, words)
    return _REFS[key]


def run(case, st, metrics0, words, use_l2=True, **kw):
    import torch
    import vllm_kvcompress_amd as kvc
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd.layout import convert_block_layout
    dev, g, fp8 = "cuda:0", st["g"], len(case) == 10
    layout = case[6] if fp8 else case[5]
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if fp8:
        q, kc, vc = st["q"].to(dev), st["k8"].to(dev), st["v8"].to(dev)
        kw.update(kv_cache_dtype=st["kind"], k_scale=st["scales"][0], v_scale=st["scales"][1])
    else:
        tdt = torch.float16 if st["dt"] == "f16" else torch.bfloat16
        t = lambda bits: torch.from_numpy(np.ascontiguousarray(bits)).to(dev).view(tdt)
        q, kc, vc = t(st["qbits"]), t(g["key_cache_bits"]), t(g["value_cache_bits"])
    out = torch.full_like(q, 7.0)                                        # (a leftover sentinel fails every comparison)
    met = None if metrics0 is None else torch.from_numpy(metrics0.copy()).to(dev)
    convert_block_layout(kc, vc, "reference", layout)
    kvc.set_block_layout(layout)
    if words is not None:
        kw["tree_mask"] = torch.from_numpy(words.view(np.int64)).to(dev)
    try:
        ops.paged_attention_kvc_chunk(out, q, kc, vc, st["Hkv"], float(g["scale"]), i32(g["block_tables"]), i32(st["ctx"]),
                                      i32(st["pos"]), i32(st["qsl"]), i32(st["qpos"]), i32(st["buf"]), st["bs"],
                                      int(st["ctx"].max()), max(st["NQ"]), metrics=met, use_l2=use_l2, **kw)
        torch.cuda.synchronize()
    finally:
        kvc.set_block_layout("reference")
    return out.float().cpu().numpy(), None if met is None else met.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case,single", RUNS)
def test_tree_matches_float64(case, single):
    fp8 = len(case) == 10
    Hq, Hkv, dt, metric, NQ = case[0], case[1], case[4], case[-3 if fp8 else -2], case[-1]
    st, words, (ref_out, ref_add, ref_hit) = tree_state(case, single)
    assert (int(st["ctx"].max()) <= st["PL"]) == single               # one partition: no combine kernel
    use_l2 = metric != "l1"
    out, added = run(case, st, None if metric is None else np.zeros_like(st["m0"]), words, use_l2)
    tol = 2e-3 if dt == "f16" else 1.6e-2
    print("max |out - ref|", np.abs(out - ref_out).max())
    assert np.allclose(out, ref_out, atol=tol * (max(1.0, st["scales"][1]) if fp8 else 1.0), rtol=tol)
    rows = np.repeat(np.arange(len(NQ)), NQ) == 4                      # fewer slots than new tokens: base < 0
    e = (np.arange(NQ[4] // 2) + (NQ[4] - NQ[4] // 2)).astype(np.uint64)
    blind = np.array([not ((w >> e) & np.uint64(1)).any() for w in words[rows]])
    assert (out[rows][blind][:, -(Hq // Hkv):] == 0).all()             # rows that see nothing: exactly 0
    if NQ[3] >= 2:                                                      # sequence 3, head 0 (base 0), token 1: word 0
        assert (out[st["qsl"][3] + 1, :Hq // Hkv] == 0).all()
        unseen = int(st["g"]["block_tables"][3, 0, 0]) * st["bs"] + 1   # its slot: no token's word has bit 1
        assert not ref_hit.reshape(-1)[unseen]
    if metric is None:
        return
    print("max rel metric error", (np.abs(added - ref_add) / np.maximum(ref_add, 1e-30))[ref_hit].max())
    assert np.allclose(added, ref_add, rtol=4e-4, atol=1e-9)           # from zeros: the store holds the added amount
    # from random values: one fp32 add of that amount per reached slot, every other slot bit-identical
    _, got = run(case, st, st["m0"], words, use_l2)
    assert np.array_equal(got[~ref_hit].view(np.int32), st["m0"][~ref_hit].view(np.int32))
    assert np.array_equal(got[ref_hit], (st["m0"] + added)[ref_hit])


@pytest.mark.gpu
@pytest.mark.parametrize("case,schedule", [(s2.CASES[0], "short"), (w2.CASES[0], "wide"), (w8.CASES[0], "wide")])
def test_chain_mask_is_the_chain_call(case, schedule):
    """only which logits are -inf depends on the mask: the chain's words give the bits of the call without a mask"""
    st = get_state(case)
    chain = np.concatenate([(np.uint64(2) << np.arange(n, dtype=np.uint64)) - np.uint64(1) for n in st["NQ"]])
    (o1, m1), (o2, m2) = (run(case, st, st["m0"], w, schedule=schedule, metric_schedule="rows") for w in (chain, None))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


@pytest.mark.gpu
def test_tree_is_deterministic():
    st, words, _ = tree_state(*RUNS[5])
    (o1, m1), (o2, m2) = (run(RUNS[5][0], st, st["m0"], words) for _ in range(2))
    assert np.array_equal(o1, o2) and np.array_equal(m1.view(np.int32), m2.view(np.int32))


def test_tree_rule_and_refusals():
    """the host side (no device needed): who is eligible, refusals before anything is launched"""
    import torch
    from vllm_kvcompress_amd import _custom_ops as ops
    from vllm_kvcompress_amd import _lib
    lib = _lib.load()
    ok = lib.kvc_paged_attention_chunk_tree_eligible
    assert [ok(64, 8, 8), ok(65, 1, 1), ok(72, 8, 8), ok(1, 1, 64), ok(1, 1, 65), ok(12, 8, 2)] == [1, 0, 0, 1, 0, 0]
    mask = (ctypes.c_uint64 * 16)()

    def error(tree=ctypes.addressof(mask), **kw):
        p = _lib.KvcAttentionChunkParams()
        p.num_seqs, p.num_tokens, p.num_heads, p.num_kv_heads, p.head_size, p.block_size = 1, 16, 8, 2, 128, 16
        p.max_query_len, p.max_context_len = 16, 16
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.kvc_paged_attention_chunk_tree(ctypes.byref(p), tree, 1.0, 1.0, None, 0, None) == 1
        return lib.kvc_last_error().decode()

    assert "tree_mask" in error(tree=None) and "tree_mask" in error(tree=ctypes.addressof(mask) + 4)
    assert "65 rows" in error(num_heads=65, num_kv_heads=1, max_query_len=1)
    assert "65 rows" in error(num_heads=1, num_kv_heads=1, max_query_len=65)       # (a word holds 64 new tokens)
    assert "head size: 96" in error(head_size=96) and "head size: 96" in error(head_size=96, kv_cache_dtype=1)
    with pytest.raises(RuntimeError, match="no tree variant"):
        ops.paged_attention_kvc_chunk(*([None] * 15), schedule="tile", tree_mask=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="int64"):
        ops.paged_attention_kvc_chunk(*([None] * 15), tree_mask=torch.zeros(4, dtype=torch.int32))
