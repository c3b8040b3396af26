"""Pair encoding (cs_tokenizer_encode_pairs: what a cross-encoder reads) against the `tokenizers` library — the version the
reference pins (Cargo.lock: tokenizers 0.22.2) — id for id, mask for mask, token type for token type: all three tokenizer
kinds under the post-processors their files come with (WordPiece with BertProcessing, byte-level BPE with RobertaProcessing
and with a TemplateProcessing pair, unigram with the XLM-R pair template), the library's default truncation (longest_first)
at lengths that cut neither, one or both bodies, bodies of 0 / 1 / 2 / 10 / 40 tokens on either side, one first text for
every pair (na = 1) and one per pair.  The fixtures are trained here with the library's own trainers (no such file is on
disk).  CPU only."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

pytest.importorskip("tokenizers")

from codesearch_amd import _lib  # noqa: E402
from codesearch_amd.tokenizer import WordPieceTokenizer  # noqa: E402

CORPUS = [
    "def authenticate(user, password):\n    return check_hash(user.password_hash, password)\n",
    "fn main() {\n    let args: Vec<String> = std::env::args().collect();\n    println!(\"{:?}\", args);\n}\n",
    "class VectorStore:\n    \"\"\"stores 384-d embeddings\"\"\"\n    def search(self, query, k=10):\n        pass\n",
    "for (int i = 0; i < 1024; ++i) { sum += a[i] * b[i]; }\n",
    "how do i authenticate users and store the password hash in the vector index\n",
] * 40
WORDS = ["user", "password", "return", "def", "search", "query", "let", "args", "main", "class", "stores", "sum", "int", "the",
         "hash", "index", "vector", "store", "how", "do", "users", "and", "in", "fn", "self", "pass"]
LENGTHS = (0, 1, 2, 10, 40)
MAX_LENGTHS = (8, 9, 12, 16, 64)
KINDS = ("wordpiece_bert", "bpe_roberta", "bpe_template", "unigram_xlmr")


def build_wordpiece(path):
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors, trainers

    tok = Tokenizer(models.WordPiece(unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(lowercase=True)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.train_from_iterator(CORPUS, trainers.WordPieceTrainer(vocab_size=400, special_tokens=["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"],
                                                              show_progress=False))
    tok.post_processor = processors.BertProcessing(sep=("[SEP]", tok.token_to_id("[SEP]")), cls=("[CLS]", tok.token_to_id("[CLS]")))
    tok.save(path)
    return Tokenizer.from_file(path)


def build(kind, path):
    if kind == "wordpiece_bert":
        return build_wordpiece(path)
    if kind.startswith("bpe"):
        import test_bpe_tokenizer as B

        return B.build(path, post="roberta" if kind == "bpe_roberta" else "template")
    pytest.importorskip("sentencepiece")
    import make_unigram_golden as G

    return G.build(path, "published", G.train())


def body_len(tok, text):
    return len(tok.encode(text, add_special_tokens=False).ids)


def text_of(tok, k, start):
    """A text of exactly k body tokens made of different words (a cut at the wrong end shows)."""
    text = ""
    for w in itertools.islice(itertools.cycle(WORDS[start:] + WORDS[:start]), 400):
        if body_len(tok, text) == k:
            break
        trial = (text + " " + w) if text else w
        if body_len(tok, trial) <= k:
            text = trial
    assert body_len(tok, text) == k, (k, text)
    return text


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    d = tmp_path_factory.mktemp("pairs")
    out = {}
    for kind in KINDS:
        path = str(d / f"{kind}.json")
        tok = build(kind, path)
        tok.no_truncation()
        firsts = [text_of(tok, k, 0) for k in LENGTHS]
        seconds = [text_of(tok, k, 7) for k in LENGTHS]
        out[kind] = (path, tok, firsts, seconds)
    return out


def library_pairs(tok, pairs, max_length, pad_id):
    tok.enable_truncation(max_length=max_length)
    tok.enable_padding(pad_id=pad_id, pad_type_id=0, pad_token=tok.id_to_token(pad_id))
    enc = tok.encode_batch(pairs)
    tok.no_truncation()
    tok.no_padding()
    return (np.array([e.ids for e in enc], np.int32), np.array([e.attention_mask for e in enc], np.int32),
            np.array([e.type_ids for e in enc], np.int32))


@pytest.mark.parametrize("max_length", MAX_LENGTHS)
@pytest.mark.parametrize("kind", KINDS)
def test_pairs_match_the_library(lib, fixtures, kind, max_length):
    path, tok, firsts, seconds = fixtures[kind]
    mine = WordPieceTokenizer.from_tokenizer_json(path, max_length=512)
    # na = n: every (first, second) combination in one call
    combos = list(itertools.product(firsts, seconds))
    want = library_pairs(tok, combos, max_length, mine.pad_id)
    got = mine.encode_pairs([a for a, _ in combos], [b for _, b in combos], max_length=max_length)
    for g, w, what in zip(got, want, ("ids", "mask", "types")):
        assert g.shape == w.shape and np.array_equal(g, w), (kind, max_length, what, np.argwhere(g != w)[:4] if g.shape == w.shape else (g.shape, w.shape))
    assert got[0].shape[1] <= max_length
    # na = 1: one first text against every second text
    for a in firsts:
        want = library_pairs(tok, [(a, b) for b in seconds], max_length, mine.pad_id)
        got = mine.encode_pairs(a, seconds, max_length=max_length)
        for g, w, what in zip(got, want, ("ids", "mask", "types")):
            assert g.shape == w.shape and np.array_equal(g, w), (kind, max_length, "na=1", what)


def test_the_truncation_table_and_the_token_types(lib, fixtures):
    """Kept (first, second) body tokens for the budgets the rule's branches fall on, and BertProcessing's type ids: 0 up to
    and including the first [SEP], 1 behind it, 0 on padding; RobertaProcessing: all 0."""
    path, tok, _, _ = fixtures["wordpiece_bert"]
    mine = WordPieceTokenizer.from_tokenizer_json(path, max_length=512)
    sep = tok.token_to_id("[SEP]")
    a10, b7, a2, b16, a7 = text_of(tok, 10, 0), text_of(tok, 7, 7), text_of(tok, 2, 0), text_of(tok, 16, 7), text_of(tok, 7, 0)
    for a, b, max_length, keep in ((a10, b7, 16, (7, 6)), (a10, b7, 12, (5, 4)), (a10, b7, 8, (3, 2)), (a2, b16, 12, (2, 7)),
                                   (a7, b7, 16, (6, 7))):
        ids, mask, types = mine.encode_pairs(a, [b, ""], max_length=max_length)
        row = ids[0][mask[0] == 1].tolist()
        first_sep = row.index(sep)
        assert (first_sep - 1, len(row) - first_sep - 2) == keep, (max_length, keep, row)
        assert types[0].tolist() == [0] * (first_sep + 1) + [1] * (len(row) - first_sep - 1)
        assert types[1][mask[1] == 0].tolist() == [0] * int((mask[1] == 0).sum())   # padding has type 0
        assert row[1:first_sep] == tok.encode(a, add_special_tokens=False).ids[:keep[0]]   # tokens come off the end
    path, tok, firsts, seconds = fixtures["bpe_roberta"]
    mine = WordPieceTokenizer.from_tokenizer_json(path, max_length=512)
    ids, mask, types = mine.encode_pairs(firsts[3], seconds, max_length=64)
    assert not types.any()
    s, e = tok.token_to_id("<s>"), tok.token_to_id("</s>")
    row = ids[2][mask[2] == 1].tolist()
    assert row[0] == s and row[-1] == e and row.count(e) == 3 and e in row[1:-1] and row[row.index(e) + 1] == e


def test_vocab_txt_handle_has_the_bert_pair_form(lib, fixtures, tmp_path):
    path, tok, firsts, seconds = fixtures["wordpiece_bert"]
    vocab = tok.get_vocab()
    p = tmp_path / "vocab.txt"
    p.write_text("\n".join(sorted(vocab, key=vocab.get)) + "\n", encoding="utf-8")
    mine = WordPieceTokenizer.from_vocab_file(str(p), lowercase=True, max_length=64)
    want = library_pairs(tok, [(firsts[3], b) for b in seconds], 16, mine.pad_id)
    got = mine.encode_pairs(firsts[3], seconds, max_length=16)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_length_query_stride_and_null_types(lib, fixtures):
    path, tok, firsts, seconds = fixtures["wordpiece_bert"]
    mine = WordPieceTokenizer.from_tokenizer_json(path, max_length=512)
    from codesearch_amd.tokenizer import pack_texts

    a_blob, a_off = pack_texts([firsts[3]])
    b_blob, b_off = pack_texts(seconds)
    L = C.c_uint32()
    args = (mine.handle, a_blob, a_off.ctypes.data_as(_lib.u64p), 1, b_blob, b_off.ctypes.data_as(_lib.u64p), len(seconds), 16)
    assert lib.cs_tokenizer_encode_pairs(*args, None, None, None, 0, C.byref(L)) == _lib.CS_OK and L.value == 16
    ids = np.full((len(seconds), 20), -7, np.int32)
    mask = np.full((len(seconds), 20), -7, np.int32)
    assert lib.cs_tokenizer_encode_pairs(*args, ids.ctypes.data_as(_lib.i32p), mask.ctypes.data_as(_lib.i32p), None, 20, C.byref(L)) == _lib.CS_OK
    want = mine.encode_pairs(firsts[3], seconds, max_length=16)
    assert np.array_equal(ids[:, :16], want[0]) and np.array_equal(mask[:, :16], want[1])
    assert (ids[:, 16:] == mine.pad_id).all() and (mask[:, 16:] == 0).all()
    rc = lib.cs_tokenizer_encode_pairs(*args, ids.ctypes.data_as(_lib.i32p), mask.ctypes.data_as(_lib.i32p), None, 15, C.byref(L))
    assert rc == _lib.CS_ERR_BAD_ARG and "row_stride" in lib.cs_last_error().decode()
    # no pairs at all
    assert lib.cs_tokenizer_encode_pairs(mine.handle, None, None, 0, None, None, 0, 16, None, None, None, 0, C.byref(L)) == _lib.CS_OK
    assert L.value == 0


def test_refusals_are_worded(lib, fixtures, tmp_path):
    path, tok, firsts, seconds = fixtures["bpe_template"]
    mine = WordPieceTokenizer.from_tokenizer_json(path, max_length=512)
    with pytest.raises(_lib.CsError) as e:      # <s> A </s> </s> B </s> adds four tokens: 5 leaves one body without any
        mine.encode_pairs(firsts[3], seconds, max_length=5)
    assert e.value.code == _lib.CS_ERR_BAD_ARG and "max_length" in str(e.value)
    assert mine.encode_pairs(firsts[3], seconds, max_length=6)[0].shape[1] == 6
    bert = WordPieceTokenizer.from_tokenizer_json(fixtures["wordpiece_bert"][0], max_length=512)
    with pytest.raises(_lib.CsError) as e:
        bert.encode_pairs(firsts[3], seconds, max_length=4)
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    with pytest.raises(ValueError):
        mine.encode_pairs(firsts[:2], seconds)
    from codesearch_amd.tokenizer import pack_texts

    a_blob, a_off = pack_texts(firsts[:2])
    b_blob, b_off = pack_texts(seconds)
    L = C.c_uint32()
    rc = lib.cs_tokenizer_encode_pairs(mine.handle, a_blob, a_off.ctypes.data_as(_lib.u64p), 2, b_blob, b_off.ctypes.data_as(_lib.u64p),
                                       len(seconds), 16, None, None, None, 0, C.byref(L))
    assert rc == _lib.CS_ERR_BAD_ARG and "first texts" in lib.cs_last_error().decode()

    doc = json.load(open(path, encoding="utf-8"))

    def create(mutate):
        d = json.loads(json.dumps(doc))
        mutate(d)
        p = str(tmp_path / "mutated.json")
        json.dump(d, open(p, "w", encoding="utf-8"), ensure_ascii=False)
        h = C.c_void_p()
        rc = lib.cs_tokenizer_create_from_json(p.encode(), 0, C.byref(h))
        return rc, h, lib.cs_last_error().decode()

    # a pair template that is neither arrangement is refused at create, as the `single` checks refuse
    rc, h, msg = create(lambda d: d["post_processor"]["pair"].pop(3))                 # <s> A </s> B </s> is fine ...
    assert rc == _lib.CS_OK, msg
    lib.cs_tokenizer_destroy(h)
    for mutate in (lambda d: d["post_processor"]["pair"].pop(),                       # ... no closing </s> is not
                   lambda d: d["post_processor"]["pair"].reverse(),
                   lambda d: d["post_processor"]["pair"].insert(0, d["post_processor"]["pair"][0]),
                   lambda d: d["post_processor"]["pair"][1]["Sequence"].__setitem__("id", "B")):
        rc, h, msg = create(mutate)
        assert rc == _lib.CS_ERR_UNSUPPORTED and "`pair`" in msg, (rc, msg)
    # the type ids are the file's
    rc, h, msg = create(lambda d: [e[next(iter(e))].__setitem__("type_id", 1) for e in d["post_processor"]["pair"][3:]])
    assert rc == _lib.CS_OK, msg
    ids = np.empty((len(seconds), 64), np.int32)
    types = np.empty((len(seconds), 64), np.int32)
    a_blob, a_off = pack_texts([firsts[2]])
    assert lib.cs_tokenizer_encode_pairs(h, a_blob, a_off.ctypes.data_as(_lib.u64p), 1, b_blob, b_off.ctypes.data_as(_lib.u64p), len(seconds),
                                         64, ids.ctypes.data_as(_lib.i32p), None, types.ctypes.data_as(_lib.i32p), 64, C.byref(L)) == _lib.CS_OK
    n_a = 1 + body_len(tok, firsts[2]) + 1
    n_b = 1 + body_len(tok, seconds[3]) + 1
    assert types[3, :L.value].tolist() == [0] * n_a + [1] * n_b + [0] * (L.value - n_a - n_b)
    lib.cs_tokenizer_destroy(h)
    # a file without a pair template, or with the bare $A $B the library writes when none was given, still loads; the pair
    # call is what refuses
    bare = [{"Sequence": {"id": "A", "type_id": 0}}, {"Sequence": {"id": "B", "type_id": 1}}]
    for mutate in (lambda d: d["post_processor"].pop("pair"), lambda d: d["post_processor"].__setitem__("pair", bare)):
        rc, h, msg = create(mutate)
        assert rc == _lib.CS_OK, msg
        rc = lib.cs_tokenizer_encode_pairs(h, a_blob, a_off.ctypes.data_as(_lib.u64p), 1, b_blob, b_off.ctypes.data_as(_lib.u64p),
                                           len(seconds), 64, None, None, None, 0, C.byref(L))
        assert rc == _lib.CS_ERR_UNSUPPORTED and "pair form" in lib.cs_last_error().decode()
        lib.cs_tokenizer_destroy(h)
