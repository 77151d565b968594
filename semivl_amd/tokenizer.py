"""CLIP's byte-level BPE tokeniser on the standard library (no `regex`, no `ftfy`).

Written from the published description of the algorithm (GPT-2's byte-level BPE as CLIP uses it): text is cleaned
(HTML-unescaped twice, whitespace collapsed, lower-cased), cut into words by a small scanner, every word is spelt in the
256 printable stand-ins of its UTF-8 bytes with `</w>` on its last symbol, and adjacent symbols are merged in the rank
order of the merges file until no ranked pair is left.

Differences from the `clip` package, by design: `ftfy`'s mojibake repair is not applied (text is taken as it is), and a text
that does not fit the context raises instead of being cut, because a cut prompt would lose the EOT position the text encoder
gathers at.
"""
import gzip
import html

import torch

SOT_TEXT, EOT_TEXT = "<|startoftext|>", "<|endoftext|>"
_CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")   # tried in this order, as the pattern's alternation
_N_MERGES = 49152 - 256 - 2                                       # CLIP's vocabulary: 49408 = 512 + 48894 + 2


def bytes_to_unicode():
    """byte value -> a printable character, GPT-2's table: the printable Latin-1 bytes stand for themselves (in the order
    '!'..'~', then 0xA1..0xAC, then 0xAE..0xFF), every other byte takes the next code point from 256 on, in ascending byte
    order.  The dict's ORDER is the vocabulary's order."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = list(bs)
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def clean(text):
    """HTML-unescape twice, collapse every whitespace run to one space, strip, lower-case."""
    text = html.unescape(html.unescape(text))
    return " ".join(text.split()).lower()


def pre_tokenize(text):
    """The words of `'s|'t|'re|'ve|'m|'ll|'d|letters+|one numeral|other non-space characters+`, left to right, on
    str.isalpha / str.isnumeric.  (CLIP's pattern also recognises the two special strings inside a text; prompts built from
    class names never hold them, and here they are spelt out like any other characters.)"""
    out, i, n = [], 0, len(text)
    while i < n:
        ch = text[i]
        if ch.isspace():
            i += 1
            continue
        hit = next((s for s in _CONTRACTIONS if text.startswith(s, i)), None)
        if hit is not None:
            out.append(hit)
            i += len(hit)
        elif ch.isalpha():
            j = i + 1
            while j < n and text[j].isalpha():
                j += 1
            out.append(text[i:j])
            i = j
        elif ch.isnumeric():
            out.append(ch)
            i += 1
        else:
            j = i + 1
            while j < n and not (text[j].isspace() or text[j].isalpha() or text[j].isnumeric()):
                j += 1
            out.append(text[i:j])
            i = j
    return out


class SimpleTokenizer:
    """`SimpleTokenizer(bpe_path)`: the merges file (gzip or plain text; first line a header; the lines after it are the
    merges, the first 48894 of them when the file is CLIP's own).  Vocabulary: the 256 byte symbols, the same with `</w>`,
    one entry per merge, then `<|startoftext|>` and `<|endoftext|>` as the last two ids."""

    def __init__(self, bpe_path):
        with open(bpe_path, "rb") as f:
            raw = f.read()
        if raw[:2] == b"\x1f\x8b":
            raw = gzip.decompress(raw)
        lines = raw.decode("utf-8").split("\n")[1:_N_MERGES + 1]
        merges = [tuple(ln.split()) for ln in lines if ln.strip()]
        for m in merges:
            if len(m) != 2:
                raise ValueError(f"SimpleTokenizer: {bpe_path}: a merge line needs two symbols, got {' '.join(m)!r}")
        self.byte_encoder = bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab] + ["".join(m) for m in merges] + [SOT_TEXT, EOT_TEXT]
        self.encoder = {s: i for i, s in enumerate(vocab)}
        self.bpe_ranks = {m: r for r, m in enumerate(merges)}
        self.vocab_size = len(vocab)
        self.sot_id, self.eot_id = self.vocab_size - 2, self.vocab_size - 1
        self._cache = {}

    def bpe(self, token):
        """symbols of one word (already in byte stand-ins) after every applicable merge"""
        if token in self._cache:
            return self._cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        inf = float("inf")
        while len(word) > 1:
            pairs = set(zip(word[:-1], word[1:]))
            best = min(pairs, key=lambda p: self.bpe_ranks.get(p, inf))
            if best not in self.bpe_ranks:
                break
            a, b = best
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == a and word[i + 1] == b:
                    merged.append(a + b)
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = tuple(merged)
        self._cache[token] = word
        return word

    def encode(self, text):
        ids = []
        for w in pre_tokenize(clean(text)):
            w = "".join(self.byte_encoder[b] for b in w.encode("utf-8"))
            ids.extend(self.encoder[s] for s in self.bpe(w))
        return ids

    def tokenize(self, texts, context_length=77):
        """int64 [n, context_length]: each row SOT, ids..., EOT, then zeros.  A text that does not fit raises ValueError."""
        if isinstance(texts, str):
            texts = [texts]
        out = torch.zeros(len(texts), context_length, dtype=torch.int64)
        for r, text in enumerate(texts):
            ids = [self.sot_id] + self.encode(text) + [self.eot_id]
            if len(ids) > context_length:
                raise ValueError(f"tokenize: {text!r} needs {len(ids)} tokens, the context holds {context_length}")
            out[r, :len(ids)] = torch.tensor(ids, dtype=torch.int64)
        return out
