"""Parity tests for the ModernBERT encoder family (cs_bert_config.arch = CS_ARCH_MODERN: the reference registry's
modernbert-embed-large entry, /root/reference/src/embed/embedder.rs:47, :72): HIP kernels through the C ABI — pre-norm layers
on the dense / attention kernels of every other family, the rotary map with a base per layer type, the local-attention window
inside the attention kernels (attention_shx_body.hpp POS = 2), the GELU gate as the up projection's epilogue — against the CPU
oracle and the committed golden vectors of HF transformers' own ModernBertModel in float64
(tests/golden/make_modern_golden.py).  Needs an MI355X.

Bar: 2e-5 against the fp32 oracle and 3e-5 against the float64 golden at 2-4 layers; at the published 28-layer shape a
random-weight network amplifies rounding by ~1.4 per layer (the fp32 ORACLE is 3.3e-5 from float64 there), so the bar is the
north star's 1e-4 against the golden."""
import json
import os

import numpy as np
import pytest

from codesearch_amd.bert_params import (ARCH_MODERN, POOL_CLS, POOL_MEAN, BertConfig, synth_params, to_state_dict,
                                        token_batch_with_lens)

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "modern_golden.npz"))
TOL_ORACLE = 2e-5
TOL_GOLDEN = 3e-5


def case_cfg(name):
    m = GOLD[name + "/meta"]
    cfg = BertConfig(vocab_size=int(m[0]), hidden=int(m[1]), layers=int(m[2]), heads=int(m[3]), intermediate=int(m[4]),
                     max_position=int(m[5]), type_vocab_size=1, pooling=POOL_MEAN, arch=ARCH_MODERN, layer_norm_eps=1e-5,
                     rotary_base=160000.0, rotary_base_local=10000.0, global_every=3, local_window=int(m[11]))
    return cfg, int(m[6]), int(m[7]), [int(x) for x in GOLD[name + "/lens"]], int(m[9])


@pytest.fixture(scope="module")
def FE(gpu_lib):
    from codesearch_amd import FastEmbedder, ModelType

    assert gpu_lib.cs_device_count() >= 1
    return lambda cfg, **kw: FastEmbedder(ModelType.ModernBertEmbedLarge, config=cfg, **kw)


@pytest.mark.parametrize("gemm_mode", ["split", "f32"])
@pytest.mark.parametrize("name", [str(n) for n in GOLD["names"] if str(n) != "modern_large_shape"])
def test_small_cases_vs_golden_and_oracle(FE, oracle, name, gemm_mode):
    cfg, wseed, iseed, lens, L = case_cfg(name)
    ids, mask = token_batch_with_lens(cfg, iseed, lens, L)
    params = synth_params(cfg, wseed)
    emb = FE(cfg, seed=wseed, gemm_mode=gemm_mode)
    got = emb.embed_ids(ids, mask)
    ref = oracle.bert_forward(cfg, params, ids, mask, want_hidden=True)
    np.testing.assert_allclose(got, ref["pooled"], atol=TOL_ORACLE)
    np.testing.assert_allclose(got, GOLD[name + "/mean"], atol=TOL_GOLDEN)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    hid = emb.last_hidden(len(lens) * L).reshape(len(lens), L, cfg.hidden)
    valid = mask.astype(bool)
    np.testing.assert_allclose(hid[valid], ref["hidden"][valid], atol=3e-4)
    split, f32, _ = emb.debug_counters()
    assert (split, f32) == ((1, 0) if gemm_mode == "split" else (0, 1))
    emb.close()


def test_published_shape_vs_golden_and_oracle(FE, oracle):
    """modernbert-embed-large's own shape (28 x 1024, 16 heads of 64, intermediate 2624 -> 2688, vocab 50368, window 64)."""
    cfg, wseed, iseed, lens, L = case_cfg("modern_large_shape")
    ids, mask = token_batch_with_lens(cfg, iseed, lens, L)
    emb = FE(cfg, seed=wseed)
    got = emb.embed_ids(ids, mask)
    ref = oracle.bert_forward(cfg, oracle.bert_synth_params(cfg, wseed), ids, mask)
    gold = GOLD["modern_large_shape/mean"]
    print("modern_large_shape: max |gpu - oracle| %.2e, |gpu - f64| %.2e, |oracle - f64| %.2e" %
          (np.abs(got - ref["pooled"]).max(), np.abs(got - gold).max(), np.abs(ref["pooled"] - gold).max()))
    np.testing.assert_allclose(got, gold, atol=1e-4)            # the north star's tolerance, against HF's float64
    np.testing.assert_allclose(got, ref["pooled"], atol=1e-4)
    assert emb.debug_counters()[:2] == (1, 0)
    emb.close()


def test_registry_entry_builds_and_runs(FE, oracle):
    """ModelType::ModernBertEmbedLarge -> the ModernBERT config (embedder.rs:72, :95: 1024 dimensions); four layers of it (one
    global, two local, one global), every dense-layer route by batch size."""
    from codesearch_amd import ModelType

    m = ModelType.ModernBertEmbedLarge
    assert (m.dimensions(), m.bert_config().arch, m.short_name()) == (1024, ARCH_MODERN, "modernbert-large")
    cfg = m.bert_config()
    cfg.layers, cfg.vocab_size = 4, 2048
    emb = FE(cfg, seed=521)
    params = synth_params(cfg, 521)
    for lens, L in (([12], 12), (list(range(96, 64, -1)), 96), ([128] * 64 + list(range(128, 64, -1)), 128)):
        ids, mask = token_batch_with_lens(cfg, 500 + len(lens), lens, L)
        got = emb.embed_ids(ids, mask)
        ref = oracle.bert_forward(cfg, params, ids, mask)["pooled"]
        np.testing.assert_allclose(got, ref, atol=TOL_ORACLE)
    assert emb.debug_counters()[1] == 0
    emb.close()


def test_padded_rows_stay_finite_and_do_not_leak(FE, oracle):
    """A padded position whose whole window is padding has no key to attend to (HF's eager softmax returns NaN there, see
    make_modern_golden.py); here the mask is finite, the padded rows are finite don't-cares and the valid rows never read
    them: a short row embeds the same alone and beside a long one."""
    cfg, wseed, iseed, _, _ = case_cfg("dh32_L100")
    L = 200
    ids, mask = token_batch_with_lens(cfg, iseed, [200, 20, 150], L)   # row 1: 180 padded positions, window 16
    emb = FE(cfg, seed=wseed)
    got = emb.embed_ids(ids, mask)
    assert np.isfinite(got).all()
    assert np.isfinite(emb.last_hidden(3 * L)).all()   # padded rows included
    # ... and on the split-f16 kernels: a NaN stored for a padded row would raise the range flag and send the whole
    # mini-batch to the exact-f32 kernels, which the pooled output cannot show
    assert emb.debug_counters()[:2] == (1, 0)
    alone = emb.embed_ids(ids[1:2, :20], mask[1:2, :20])
    np.testing.assert_allclose(got[1], alone[0], atol=2e-6)
    ref = oracle.bert_forward(cfg, synth_params(cfg, wseed), ids, mask)["pooled"]
    np.testing.assert_allclose(got, ref, atol=TOL_ORACLE)
    assert emb.debug_counters()[1] == 0
    emb.close()


@pytest.mark.parametrize("hidden,heads,window", [(384, 12, 16), (1024, 16, 64)])
def test_published_lengths_with_ragged_rows(FE, oracle, hidden, heads, window):
    """The lengths the published model runs to (L = 300, 512), three layers (global, local, local), one full row, one that
    crosses 256 tokens and one short row: beyond 256 tokens a block of the local layers skips the 128-key super-tiles no
    query of it can see, and the short row leaves whole query blocks without a visible key."""
    cfg = BertConfig(vocab_size=1024, hidden=hidden, layers=3, heads=heads, intermediate=1536, max_position=512, type_vocab_size=1,
                     pooling=POOL_MEAN, arch=ARCH_MODERN, layer_norm_eps=1e-5, rotary_base=160000.0, rotary_base_local=10000.0,
                     global_every=3, local_window=window)
    wseed = 700 + hidden
    params = synth_params(cfg, wseed)
    emb = FE(cfg, seed=wseed)
    for n, (L, lens) in enumerate(((300, [300, 270, 30]), (512, [512, 290, 40]))):
        ids, mask = token_batch_with_lens(cfg, 800 + L, lens, L)
        got = emb.embed_ids(ids, mask)
        ref = oracle.bert_forward(cfg, params, ids, mask)["pooled"]
        print("modern %d x %d heads, window %d, L %d: max |gpu - oracle| %.2e" % (hidden, heads, window, L, np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, atol=TOL_ORACLE)
        np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
        assert emb.debug_counters()[:2] == (n + 1, 0)
    emb.close()


def modern_snapshot(d, cfg, flat, file_intermediate=None):
    """A ModernBERT snapshot directory: config.json with HF's keys and model.safetensors with ModernBertModel's names, no
    biases anywhere (the published arrangement), the feed-forward at `file_intermediate` columns (the published 2,624 against
    the config's padded width)."""
    from safetensors.numpy import save_file

    os.makedirs(d, exist_ok=True)
    If = file_intermediate or cfg.intermediate
    hf = {"model_type": "modernbert", "architectures": ["ModernBertModel"], "vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden,
          "num_hidden_layers": cfg.layers, "num_attention_heads": cfg.heads, "intermediate_size": If, "max_position_embeddings": 8192,
          "norm_eps": cfg.layer_norm_eps, "norm_bias": False, "attention_bias": False, "mlp_bias": False, "hidden_activation": "gelu",
          "global_attn_every_n_layers": cfg.global_every, "local_attention": 2 * cfg.local_window, "global_rope_theta": cfg.rotary_base,
          "local_rope_theta": cfg.rotary_base_local, "classifier_pooling": "mean"}
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(hf, f)
    ours = to_state_dict(cfg, flat)
    sd = {"embeddings.tok_embeddings.weight": ours["embeddings.word_embeddings.weight"], "embeddings.norm.weight": ours["embeddings.LayerNorm.weight"],
          "final_norm.weight": ours["final_norm.weight"]}
    for l in range(cfg.layers):
        a, b = f"encoder.layer.{l}.", f"layers.{l}."
        if l:
            sd[b + "attn_norm.weight"] = ours[a + "attention.output.LayerNorm.weight"]
        sd[b + "attn.Wqkv.weight"] = np.concatenate([ours[a + f"attention.self.{r}.weight"] for r in ("query", "key", "value")])
        sd[b + "attn.Wo.weight"] = ours[a + "attention.output.dense.weight"]
        sd[b + "mlp_norm.weight"] = ours[a + "output.LayerNorm.weight"]
        sd[b + "mlp.Wi.weight"] = np.concatenate([ours[a + "intermediate.gate.weight"][:If], ours[a + "intermediate.dense.weight"][:If]])
        sd[b + "mlp.Wo.weight"] = ours[a + "output.dense.weight"][:, :If]
    save_file({"model." + k: np.ascontiguousarray(v) for k, v in sd.items()}, os.path.join(d, "model.safetensors"))


def test_embedder_from_a_modernbert_snapshot_directory(FE, oracle, tmp_path):
    """cs_embedder_create_from_dir on a ModernBERT snapshot whose feed-forward is narrower than the kernels' tile (I_f = 2,624
    = 20.5 x 128 in the published model; 1,472 = 11.5 x 128 here): the loader pads with zero rows / columns, and the
    embedder equals one handed the padded block — and the oracle."""
    from codesearch_amd import FastEmbedder
    from codesearch_amd.pipeline import synth_vocab

    cfg = BertConfig(vocab_size=1024, hidden=1024, layers=3, heads=16, intermediate=1536, max_position=512, type_vocab_size=1,
                     pooling=POOL_MEAN, arch=ARCH_MODERN, layer_norm_eps=1e-5, rotary_base=160000.0, rotary_base_local=10000.0,
                     global_every=3, local_window=64)
    If = 1472
    flat = synth_params(cfg, 85)
    sd = to_state_dict(cfg, flat)   # views: zero what the published arrangement does not have / the padding must be
    for name, a in sd.items():
        if name.endswith(".bias"):
            a[:] = 0
    for l in range(cfg.layers):
        p = f"encoder.layer.{l}."
        sd[p + "intermediate.dense.weight"][If:] = 0
        sd[p + "intermediate.gate.weight"][If:] = 0
        sd[p + "output.dense.weight"][:, If:] = 0
    sd["encoder.layer.0.attention.output.LayerNorm.weight"][:] = 1   # (layer 0's attn_norm slot: never read)
    d = tmp_path / "snapshot"
    modern_snapshot(str(d), cfg, flat, file_intermediate=If)
    vocab = synth_vocab(1024)
    (d / "vocab.txt").write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n")
    emb = FastEmbedder.from_dir(str(d))
    assert (emb.config.arch, emb.dimensions(), emb.config.intermediate, emb.config.local_window, emb.config.global_every,
            emb.config.pooling) == (ARCH_MODERN, 1024, 1536, 64, 3, POOL_MEAN)
    ids, mask = token_batch_with_lens(cfg, 911, [90, 60, 33], 90)
    got = emb.embed_ids(ids, mask)
    ref_emb = FE(cfg, params=flat)
    assert np.array_equal(got, ref_emb.embed_ids(ids, mask))
    np.testing.assert_allclose(got, oracle.bert_forward(cfg, flat, ids, mask)["pooled"], atol=TOL_ORACLE)
    emb.close()
    ref_emb.close()


def test_embedder_from_a_fastembed_cache_of_the_onnx_export(FE, tmp_path):
    """What fastembed leaves on disk for the registry entry: config.json + onnx/model.onnx (no safetensors).  The file is
    written here by torch.onnx's exporter from transformers' own ModernBertModel (tests/golden/make_modern_onnx_fixture.py) at
    a width the kernels run (hidden 384, 12 heads, 3 layers, feed-forward 200 inside a block padded to 256, local window 8
    either side); the embedder loaded from it must reproduce the EXPORTING MODEL's own pooled output on a padded batch
    longer than the local window."""
    import importlib.util

    from codesearch_amd import FastEmbedder

    spec = importlib.util.spec_from_file_location("make_modern_onnx_fixture", os.path.join(os.path.dirname(__file__), "golden", "make_modern_onnx_fixture.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = tmp_path / "cache"
    (d / "onnx").mkdir(parents=True)
    mod.write(str(d / "onnx"), "model", dims=(384, 12, 3, 200, 64), local_attention=16)
    state = np.load(str(d / "onnx" / "model_state.npz"))
    hf = {"model_type": "modernbert", "architectures": ["ModernBertModel"], "vocab_size": 64, "hidden_size": 384, "num_hidden_layers": 3,
          "num_attention_heads": 12, "intermediate_size": 200, "max_position_embeddings": 64, "norm_eps": 1e-5, "norm_bias": False,
          "attention_bias": False, "mlp_bias": False, "hidden_activation": "gelu", "global_attn_every_n_layers": 3, "local_attention": 16,
          "global_rope_theta": 160000.0, "local_rope_theta": 10000.0, "classifier_pooling": "mean"}
    (d / "config.json").write_text(json.dumps(hf))
    (d / "vocab.txt").write_text("\n".join(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(59)]) + "\n")
    emb = FastEmbedder.from_dir(str(d))
    assert (emb.config.arch, emb.dimensions(), emb.config.intermediate, emb.config.local_window, emb.config.pooling) == (ARCH_MODERN, 384, 256, 8, POOL_MEAN)
    got = emb.embed_ids(state["query_ids"], state["query_mask"])
    np.testing.assert_allclose(got, state["query_pooled"], atol=TOL_GOLDEN)
    emb.close()
