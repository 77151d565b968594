"""`python -m semivl_amd.tools.text_embeddings --clip FILE --bpe FILE --classes classes.json --variant V --out NAME.npy`

Text embeddings for any class list: the reference's model/text_embeddings.py:156-186 (`single_template`,
`single_template_concept_avg`) without the `clip` package: the tokeniser is semivl_amd/tokenizer.py, the text tower runs on
the HIP kernel library (model/text_encoder.py).

  --clip      the CLIP archive (ViT-B-16.pt), a plain CLIP state dict, or the file `convert_clip_weights --text` wrote
  --bpe       CLIP's merges file (bpe_simple_vocab_16e6.txt.gz, or the same unpacked)
  --classes   JSON: a list of names, or a list of lists whose first entry is the class name and whose entries are the
              class's concepts (the shape of VOC12_wbg_classes_w_concepts4)
  --variant   single      one row per class (with lists: the first entry)
              concept     one row per concept, classes in order, plus NAME.concepts.json {"counts": [...]}, which
                          model.text_embeddings.get_class_to_concept_idxs reads for the per-class maximum
              conceptavg  the un-normalised concept embeddings averaged per class, then L2-normalised
  --template  default "a photo of a {}"

The output is float32 [rows, embed] with unit rows, like the shipped files.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from ..checkpoint import load_clip_archive
from ..model.text_embeddings import class_to_concept_idxs_from_counts, concept_offsets, sidecar_path
from ..model.text_encoder import CLIPTextEncoder
from ..tokenizer import SimpleTokenizer
from .. import ops

VARIANTS = ("single", "concept", "conceptavg")


def read_classes(path):
    """-> list of concept lists (a plain name is its own only concept)"""
    with open(path) as f:
        data = json.load(f)
    if not isinstance(data, list) or not data:
        raise ValueError(f"{path}: expected a non-empty JSON list")
    out = []
    for i, entry in enumerate(data):
        if isinstance(entry, str):
            entry = [entry]
        if not isinstance(entry, list) or not entry or not all(isinstance(s, str) and s for s in entry):
            raise ValueError(f"{path}: entry {i} must be a name or a non-empty list of names, got {entry!r}")
        out.append(list(entry))
    return out


def prompts_for(classes, variant, template):
    """(prompts, counts): counts is None for `single`, else the number of concepts of each class"""
    if variant == "single":
        return [template.format(c[0]) for c in classes], None
    return [template.format(s) for c in classes for s in c], [len(c) for c in classes]


def embed(encoder, tokenizer, classes, variant, template="a photo of a {}"):
    """float32 [rows, embed] on the encoder's device, unit rows; and the concept counts (None for `single`)"""
    if variant not in VARIANTS:
        raise ValueError(f"variant {variant!r} is none of {VARIANTS}")
    prompts, counts = prompts_for(classes, variant, template)
    tokens = tokenizer.tokenize(prompts, context_length=encoder.context_length)
    if variant != "conceptavg":
        return encoder.encode(tokens, normalize=True), counts
    raw = encoder.encode(tokens, normalize=False)
    offs = concept_offsets(class_to_concept_idxs_from_counts(counts), raw.device)
    out, _ = ops.l2norm_fwd(ops.segment_mean(raw, offs))      # the mean first, then the norm (text_embeddings.py:178-183)
    return out, counts


def main(argv=None):
    ap = argparse.ArgumentParser(description="CLIP text embeddings for a class list")
    ap.add_argument("--clip", required=True)
    ap.add_argument("--bpe", required=True)
    ap.add_argument("--classes", required=True)
    ap.add_argument("--variant", required=True, choices=VARIANTS)
    ap.add_argument("--out", required=True)
    ap.add_argument("--template", default="a photo of a {}")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools.text_embeddings: the text tower runs on the GPU (there is no host path)")
    out_path = a.out if a.out.endswith(".npy") else a.out + ".npy"
    classes = read_classes(a.classes)
    tok = SimpleTokenizer(a.bpe)
    sd = load_clip_archive(a.clip)
    enc = CLIPTextEncoder.from_clip_state_dict(sd).to("cuda:0")
    if tok.vocab_size != enc.vocab_size:
        raise ValueError(f"--bpe gives a vocabulary of {tok.vocab_size}, the text tower embeds {enc.vocab_size}")
    t0 = time.perf_counter()
    out, counts = embed(enc, tok, classes, a.variant, a.template)
    arr = out.cpu().numpy().astype(np.float32)
    dt = time.perf_counter() - t0
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.save(out_path, arr)
    if a.variant == "concept":
        with open(sidecar_path(out_path), "w") as f:
            json.dump({"counts": counts}, f)
    print(f"{out_path}: {arr.shape[0]} x {arr.shape[1]} ({a.variant}), tokenise + encode {dt * 1e3:.1f} ms")


if __name__ == "__main__":
    main()
