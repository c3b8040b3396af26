// pair_form.hpp — how a tokenizer handle arranges a (first text, second text) pair: the post-processor's pair template, as
// far as cs_tokenizer_encode_pairs restates it.  Two arrangements exist in the models this library runs:
//   BERT     [CLS] A [SEP] B [SEP]          (BertProcessing; a TemplateProcessing file spells it out, type ids included)
//   ROBERTA  <s> A </s> </s> B </s>         (RobertaProcessing: every type id 0)
// types[i] is the token-type id of piece i of the arrangement (a body's tokens all carry its piece's id).
#pragma once
#include <cstdint>

namespace cs {

struct PairForm {
    enum Kind { NONE = -1, BERT = 0, ROBERTA = 1 };
    int kind = NONE;                          // NONE: the file's post-processor has no pair form this library restates
    int32_t types[6] = {0, 0, 0, 0, 0, 0};    // BERT: cls A sep B sep; ROBERTA: bos A eos eos B eos
    uint32_t added() const { return kind == BERT ? 3u : 4u; }   // tokens the template adds
    static PairForm bert() { PairForm p; p.kind = BERT; p.types[3] = p.types[4] = 1; return p; }   // BertProcessing's type ids
    static PairForm roberta() { PairForm p; p.kind = ROBERTA; return p; }
};

}  // namespace cs
