"""CPU: semivl_amd/tokenizer.py against the specification of CLIP's byte-level BPE, on a synthetic merge table written here
(CLIP's own merges file is not part of the repository).  The last test compares a few prompts against the real file when the
environment variable SVL_CLIP_BPE names it."""
import gzip
import os

import pytest
import torch

from semivl_amd.tokenizer import SimpleTokenizer, bytes_to_unicode, clean, pre_tokenize

# rank order matters: ("t", "h") before ("h", "e</w>"), so "the" -> th + e</w> -> the</w>, never t + he</w>
MERGES = [("t", "h"), ("h", "e</w>"), ("th", "e</w>"), ("a", "b"), ("ab", "c</w>"), ("p", "h"), ("o", "t"), ("ph", "ot"),
          ("o", "f</w>"), ("a", "n"), ("i", "n"), ("in", "g</w>"), ("c", "a"), ("ca", "t</w>"), ("d", "o"), ("do", "g</w>"),
          ("'", "t</w>"), ("1", "2"), ("é", "e"), ("o</w>", "x"), ("n", "'")]


def write_merges(path, zipped):
    text = "#version: synthetic\n" + "\n".join(" ".join(m) for m in MERGES) + "\n"
    if zipped:
        with gzip.open(path, "wb") as f:
            f.write(text.encode("utf-8"))
    else:
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
    return path


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    return SimpleTokenizer(write_merges(str(tmp_path_factory.mktemp("bpe") / "merges.txt"), False))


def names(tok, ids):
    inv = {i: s for s, i in tok.encoder.items()}
    return [inv[i] for i in ids]


def test_vocabulary_layout(tok):
    assert tok.vocab_size == 512 + len(MERGES) + 2 == len(tok.encoder)
    assert (tok.sot_id, tok.eot_id) == (tok.vocab_size - 2, tok.vocab_size - 1)
    assert tok.encoder["<|startoftext|>"] == tok.sot_id and tok.encoder["<|endoftext|>"] == tok.eot_id
    # byte symbols in GPT-2's order: '!' .. '~', 0xA1 .. 0xAC, 0xAE .. 0xFF, then the remaining bytes from code point 256
    assert tok.encoder["!"] == 0 and tok.encoder["a"] == ord("a") - ord("!") == 64
    assert tok.encoder["a</w>"] == 256 + 64 and tok.encoder["!</w>"] == 256
    assert tok.encoder["~"] == 93 and tok.encoder["¡"] == 94 and tok.encoder["®"] == 94 + 12
    b2u = bytes_to_unicode()
    assert len(b2u) == 256 and len(set(b2u.values())) == 256
    assert b2u[0] == chr(256) and b2u[32] == chr(256 + 32) and b2u[0xAD] == chr(256 + 67) and tok.encoder[b2u[0]] == 188
    assert b2u[0xC3] == "Ã" and tok.encoder["Ã"] == 94 + 12 + (0xC3 - 0xAE)      # a non-ASCII byte
    for r, m in enumerate(MERGES):
        assert tok.encoder["".join(m)] == 512 + r


def test_merges_in_rank_order_and_inside_words_only(tok):
    assert names(tok, tok.encode("the")) == ["the</w>"]                # t h e</w> -> th e</w> -> the</w> (rank 0, then 2)
    assert names(tok, tok.encode("he")) == ["he</w>"]                  # rank 1 applies where rank 0 does not
    assert names(tok, tok.encode("abc")) == ["abc</w>"]
    assert names(tok, tok.encode("abab")) == ["ab", "a", "b</w>"]      # (a, b) does not match (a, b</w>)
    assert names(tok, tok.encode("photo")) == ["phot", "o</w>"]        # p h o t o</w>: ph, ot, then ph + ot
    assert names(tok, tok.encode("t he")) == ["t</w>", "he</w>"]       # no merge across the word boundary
    assert names(tok, tok.encode("o x")) == ["o</w>", "x</w>"]         # although ("o</w>", "x") is a ranked pair
    assert names(tok, tok.encode("cat dog")) == ["cat</w>", "dog</w>"]


def test_end_of_word_mark_only_on_the_last_symbol(tok):
    for text in ("a photo of a cat", "thethe abcabc", "xyzzy!?", "é1"):
        for word in pre_tokenize(clean(text)):
            syms = tok.bpe("".join(tok.byte_encoder[b] for b in word.encode("utf-8")))
            assert syms[-1].endswith("</w>") and not any("</w>" in s for s in syms[:-1]), (word, syms)


def test_cleaning_and_word_split(tok):
    assert clean("  A  Photo\tOF\n a   CAT ") == "a photo of a cat"
    assert clean("cats &amp;amp; dogs &lt;3") == "cats & dogs <3"         # unescaped twice
    assert tok.encode("The   CAT") == tok.encode("the cat")
    assert pre_tokenize("don't") == ["don", "'t"]
    assert names(tok, tok.encode("don't")) == ["do", "n</w>", "'t</w>"]     # ("n", "'") is ranked, but across words
    assert pre_tokenize("it's we'll they've i'm you'd we're") == ["it", "'s", "we", "'ll", "they", "'ve", "i", "'m", "you", "'d",
                                                                  "we", "'re"]
    assert pre_tokenize("a-b, (c)!!") == ["a", "-", "b", ",", "(", "c", ")!!"]
    assert pre_tokenize("x'") == ["x", "'"]


def test_each_digit_stands_alone(tok):
    assert pre_tokenize("route 66b 1a2") == ["route", "6", "6", "b", "1", "a", "2"]
    assert names(tok, tok.encode("12")) == ["1</w>", "2</w>"]          # although ("1", "2") is a ranked pair
    assert pre_tokenize("½①") == ["½", "①"]          # other numerals too


def test_non_ascii_goes_through_utf8_bytes(tok):
    ids = tok.encode("é")
    b2u = bytes_to_unicode()
    assert names(tok, ids) == [b2u[0xC3], b2u[0xA9] + "</w>"]
    assert names(tok, tok.encode("éa")) == [b2u[0xC3], b2u[0xA9], "a</w>"]
    assert tok.encode("<|endoftext|>") != [tok.eot_id]          # inside a text the special strings are ordinary characters


def test_row_layout_padding_and_context_length(tok):
    rows = tok.tokenize(["a photo of a cat", "dog"])
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (2, 77)
    for r, text in enumerate(["a photo of a cat", "dog"]):
        ids = tok.encode(text)
        assert rows[r, 0] == tok.sot_id and rows[r, 1:1 + len(ids)].tolist() == ids and rows[r, 1 + len(ids)] == tok.eot_id
        assert (rows[r, 2 + len(ids):] == 0).all()
        assert int(rows[r].argmax()) == 1 + len(ids)              # the EOT is the row's first maximum
    assert tuple(tok.tokenize("dog").shape) == (1, 77)
    short = tok.tokenize(["the cat"], context_length=4)
    assert short.tolist() == [[tok.sot_id, tok.encoder["the</w>"], tok.encoder["cat</w>"], tok.eot_id]]
    assert tuple(tok.tokenize(["the"], context_length=192).shape) == (1, 192)


def test_overflow_raises_and_quotes_the_text(tok):
    with pytest.raises(ValueError, match="the cat dog"):
        tok.tokenize(["the", "the cat dog"], context_length=4)
    long = " ".join(["cat"] * 76)
    with pytest.raises(ValueError, match="78 tokens"):
        tok.tokenize([long])
    assert tok.tokenize([" ".join(["cat"] * 75)])[0, 76] == tok.eot_id


def test_gzip_and_plain_files_load_alike(tok, tmp_path):
    tz = SimpleTokenizer(write_merges(str(tmp_path / "merges.txt.gz"), True))
    assert tz.encoder == tok.encoder and tz.bpe_ranks == tok.bpe_ranks
    text = "a photo of the dog's 12 cats, don't"
    assert tz.encode(text) == tok.encode(text)


def test_deterministic(tok, tmp_path):
    other = SimpleTokenizer(write_merges(str(tmp_path / "again.txt"), False))
    texts = ["a photo of a cat", "the photographing dog", "don't", "é 12"]
    a, b, c = tok.tokenize(texts), tok.tokenize(texts), other.tokenize(texts)
    assert torch.equal(a, b) and torch.equal(a, c)


def test_bad_merge_line_is_refused(tmp_path):
    p = tmp_path / "bad.txt"
    p.write_text("#version\nt h\nlonely\n", encoding="utf-8")
    with pytest.raises(ValueError, match="lonely"):
        SimpleTokenizer(str(p))


def test_real_clip_merges_file_when_given():
    """Against ids published with CLIP (`clip.tokenize` of these prompts).  Needs CLIP's bpe_simple_vocab_16e6.txt.gz, which is
    not in the repository: set SVL_CLIP_BPE to its path.  NOT RUN when this was written: no copy of the file was at hand."""
    path = os.environ.get("SVL_CLIP_BPE")
    if not path:
        pytest.skip("SVL_CLIP_BPE is not set")
    t = SimpleTokenizer(path)
    assert t.vocab_size == 49408 and (t.sot_id, t.eot_id) == (49406, 49407)
    assert t.tokenize(["a photo of a cat"])[0, :7].tolist() == [49406, 320, 1125, 539, 320, 2368, 49407]
    assert t.tokenize(["a photo of a dog"])[0, :7].tolist() == [49406, 320, 1125, 539, 320, 1929, 49407]
    assert t.tokenize(["a diagram"])[0, :4].tolist() == [49406, 320, 22697, 49407]
    assert t.tokenize(["hello world!"])[0, :5].tolist() == [49406, 3306, 1002, 256, 49407]
