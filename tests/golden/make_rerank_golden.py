#!/usr/bin/env python3
"""An independent golden for the cross-encoder (tests/test_gpu_rerank.py): HF transformers' BertForSequenceClassification
in float64 on the CPU — a two-layer BGE-small-shaped BERT with the library's synthetic weights (bert_params.synth_params)
and a seeded head (numpy default_rng: W_p, w_c ~ N(0, 0.05), biases ~ N(0, 0.1)) — scoring real pair encodings with token
types, written by the `tokenizers` library under BertProcessing.  Writes tests/golden/rerank_golden.npz: the inputs, the
logits and the seeds (a few KB).

    python tests/golden/make_rerank_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PARAM_SEED, HEAD_SEED, LAYERS, MAX_POSITION, VOCAB = 2024, 77, 2, 64, 512

QUERY = "how do i pad a batch"
DOCUMENTS = ["pad the batch to the longest row", "fn main ( ) { let v = vec ! [ 1 , 2 ] ; }", "", "zeta",
             "a much longer document that is cut by the truncation of the pair because it goes on and on and on well past "
             "the sixty four tokens the model was built for so that the longest first rule has something to take away",
             "do i pad"]


def seeded_head(seed, hidden=384):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 0.05, (hidden, hidden)).astype(np.float32), rng.normal(0, 0.1, hidden).astype(np.float32),
            rng.normal(0, 0.05, hidden).astype(np.float32), rng.normal(0, 0.1, 1).astype(np.float32))


def main():
    import torch
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors
    from transformers import BertConfig as HfConfig
    from transformers import BertForSequenceClassification

    from codesearch_amd.bert_params import POOL_CLS, BertConfig, synth_params, to_state_dict
    from codesearch_amd.pipeline import synth_vocab

    vocab = synth_vocab(VOCAB)
    tk = Tokenizer(models.WordPiece(vocab, unk_token="[UNK]", max_input_chars_per_word=100))
    tk.normalizer = normalizers.BertNormalizer(lowercase=True)
    tk.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tk.post_processor = processors.BertProcessing(sep=("[SEP]", vocab["[SEP]"]), cls=("[CLS]", vocab["[CLS]"]))
    tk.enable_truncation(max_length=MAX_POSITION)
    tk.enable_padding(pad_id=vocab["[PAD]"], pad_type_id=0, pad_token="[PAD]")
    enc = tk.encode_batch([(QUERY, d) for d in DOCUMENTS])
    ids = np.array([e.ids for e in enc], np.int32)
    mask = np.array([e.attention_mask for e in enc], np.int32)
    types = np.array([e.type_ids for e in enc], np.int32)

    cfg = BertConfig(vocab_size=VOCAB, hidden=384, layers=LAYERS, heads=12, intermediate=1536, max_position=MAX_POSITION, pooling=POOL_CLS)
    head = seeded_head(HEAD_SEED)
    hf = HfConfig(vocab_size=VOCAB, hidden_size=384, num_hidden_layers=LAYERS, num_attention_heads=12, intermediate_size=1536,
                  max_position_embeddings=MAX_POSITION, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu", num_labels=1,
                  hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = BertForSequenceClassification(hf)
    sd = {"bert." + k: torch.from_numpy(np.array(v)) for k, v in to_state_dict(cfg, synth_params(cfg, PARAM_SEED)).items()}
    sd.update({"bert.pooler.dense.weight": torch.from_numpy(head[0]), "bert.pooler.dense.bias": torch.from_numpy(head[1]),
               "classifier.weight": torch.from_numpy(head[2][None, :]), "classifier.bias": torch.from_numpy(head[3])})
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    model = model.double().eval()
    with torch.no_grad():
        logits = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long(),
                       token_type_ids=torch.from_numpy(types).long()).logits[:, 0].numpy()
    import tokenizers
    import transformers

    np.savez(os.path.join(HERE, "rerank_golden.npz"), ids=ids, mask=mask, types=types, logits=logits, param_seed=PARAM_SEED,
             head_seed=HEAD_SEED, layers=LAYERS, max_position=MAX_POSITION, vocab_size=VOCAB,
             made_with=np.array(f"transformers {transformers.__version__}, tokenizers {tokenizers.__version__}, torch {torch.__version__}"))
    print("logits", logits, "shape", ids.shape, "type-1 tokens", int(types.sum()))


if __name__ == "__main__":
    main()
