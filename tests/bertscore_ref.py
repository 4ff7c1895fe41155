"""CPU restatement of bert_score's pipeline (bert_score 0.3.x, idf=False, all_layers=False) for the BERTScore tests, and the fp32 trunk oracle
(`transformers.RobertaModel`). Not a conftest: imported by the test modules that need it.

  * `greedy_cos_idf`: bert_score.utils.greedy_cos_idf -- embeddings normalised, sim = bmm(hyp, ref^T) times the padding mask, row / column maxima,
    idf-weighted means, F = 2PR / (P + R), empty (length-2) sides -> P = R = 0 after F was formed, NaN F -> 0;
  * `bert_cos_score`: bert_cos_score_idf's second half -- chunks of `batch_size` consecutive pairs, each side padded with 2.0 to the chunk's
    longest sentence (pad_sequence(padding_value=2.0)) and a length mask;
  * `rescale`: (x - b) / (1 - b).
"""
from collections import OrderedDict

import numpy as np
import torch


def greedy_cos_idf(ref_embedding, ref_masks, ref_idf, hyp_embedding, hyp_masks, hyp_idf):
    ref_embedding = ref_embedding / torch.norm(ref_embedding, dim=-1).unsqueeze(-1)
    hyp_embedding = hyp_embedding / torch.norm(hyp_embedding, dim=-1).unsqueeze(-1)
    sim = torch.bmm(hyp_embedding, ref_embedding.transpose(1, 2))
    masks = torch.bmm(hyp_masks.unsqueeze(2).to(sim.dtype), ref_masks.unsqueeze(1).to(sim.dtype))
    sim = sim * masks
    word_precision = sim.max(dim=2)[0]
    word_recall = sim.max(dim=1)[0]
    hyp_idf = hyp_idf / hyp_idf.sum(dim=1, keepdim=True)
    ref_idf = ref_idf / ref_idf.sum(dim=1, keepdim=True)
    P = (word_precision * hyp_idf).sum(dim=1)
    R = (word_recall * ref_idf).sum(dim=1)
    F = 2 * P * R / (P + R)
    hyp_zero = hyp_masks.sum(dim=1).eq(2)
    ref_zero = ref_masks.sum(dim=1).eq(2)
    P, R = P.masked_fill(hyp_zero, 0.0), R.masked_fill(hyp_zero, 0.0)
    P, R = P.masked_fill(ref_zero, 0.0), R.masked_fill(ref_zero, 0.0)
    F = F.masked_fill(torch.isnan(F), 0.0)
    return P, R, F


def _pad_batch(stats):
    emb, idf = zip(*stats)
    lens = [e.shape[0] for e in emb]
    emb_pad = torch.nn.utils.rnn.pad_sequence(list(emb), batch_first=True, padding_value=2.0)
    idf_pad = torch.nn.utils.rnn.pad_sequence(list(idf), batch_first=True)
    base = torch.arange(max(lens)).expand(len(lens), max(lens))
    return emb_pad, base < torch.tensor(lens).unsqueeze(1), idf_pad


def bert_cos_score(stats, refs, hyps, batch_size):
    """stats: sentence -> (embedding [L, D], idf [L]) -> (P, R, F) [n] in the dtype of the embeddings."""
    out = []
    for lo in range(0, len(refs), batch_size):
        r = _pad_batch([stats[s] for s in refs[lo:lo + batch_size]])
        h = _pad_batch([stats[s] for s in hyps[lo:lo + batch_size]])
        out.append(torch.stack(greedy_cos_idf(*r, *h), -1))
    out = torch.cat(out)
    return out[:, 0], out[:, 1], out[:, 2]


def rescale(x, b):
    return (x - b) / (1 - b)


class WordTokenizer:
    """A stand-in for the roberta-large tokenizer (not available offline) with the surface bert_score's sent_encode uses: words hash to ids in
    [3, vocab), `<s>` = 0, `<pad>` = 1, `</s>` = 2, truncation to model_max_length including the two special tokens."""
    cls_token_id, pad_token_id, sep_token_id = 0, 1, 2

    def __init__(self, vocab=1000, model_max_length=512):
        self.vocab, self.model_max_length = vocab, model_max_length

    def _id(self, word):
        h = 0
        for ch in word:
            h = (h * 131 + ord(ch)) % 1000003
        return 3 + h % (self.vocab - 3)

    def build_inputs_with_special_tokens(self, ids):
        return [self.cls_token_id] + list(ids) + [self.sep_token_id]

    def encode(self, text, add_special_tokens=True, add_prefix_space=False, max_length=None, truncation=False):
        assert add_special_tokens and add_prefix_space
        ids = [self._id(w) for w in text.split()]
        if truncation and max_length is not None:
            ids = ids[:max_length - 2]
        return self.build_inputs_with_special_tokens(ids)


def hf_roberta(cfg, engine_sd, num_layers=None):
    """transformers.RobertaModel (fp32, eval, no pooler) holding the engine-named weights `engine_sd` (bert.embeddings.* / bert.encoder.*)."""
    import transformers
    n = cfg.num_hidden_layers if num_layers is None else num_layers
    hc = transformers.RobertaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=n,
                                    num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                                    max_position_embeddings=cfg.max_position_embeddings, type_vocab_size=cfg.type_vocab_size,
                                    layer_norm_eps=cfg.layer_norm_eps, pad_token_id=cfg.pad_token_id, hidden_act="gelu")
    hc._attn_implementation = "eager"
    m = transformers.RobertaModel(hc, add_pooling_layer=False).eval()
    sd = OrderedDict((k[len("bert."):], v.float()) for k, v in engine_sd.items() if k.startswith("bert."))
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all("position_ids" in k or "token_type_ids" in k for k in missing), (missing, unexpected)
    return m


def trunk_stats(model, toks, idf_of):
    """bert_score's get_bert_embedding per sentence on the oracle trunk: token lists -> [(embedding [L, D] fp64, idf [L] fp64)]."""
    out = []
    with torch.no_grad():
        for t in toks:
            ids = torch.tensor([t], dtype=torch.int64)
            h = model(ids, attention_mask=torch.ones_like(ids)).last_hidden_state[0].double()
            out.append((h, torch.tensor([idf_of(i) for i in t], dtype=torch.float64)))
    return out


def np_f64(x):
    return np.asarray(x, dtype=np.float64)
