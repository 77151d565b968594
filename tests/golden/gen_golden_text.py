"""Golden-vector generator for CLIP's text tower (third_party/zegclip/models/backbones/text_encoder.py:22-87).  Runs ONLY in
the build container, like gen_golden.py: it builds the reference's own CLIPTextEncoder through tests/golden/_ref_shim.py, runs it
in FLOAT64 and writes tests/golden/text_encoder.npz:

    dims            context_length 9, vocab_size 40, transformer_width 128, transformer_heads 2, transformer_layers 2, embed_dim 32
    w/<key>         the weights under CLIP's own keys, fp16: seeded draws (tests/text_ref.py: seeded_clip_text_state) rounded
                    to multiples of 2^-7, so that fp16 holds them exactly and the file stays small; every run below uses
                    exactly these values
    tokens          int64 [5, 9]: sequences of 2 .. 6 tokens, SOT = 38 first, EOT = 39 last, zero padding
    raw, out        the reference's float64 output [5, 32], and the same with unit rows
    counts, avg     the grouping [2, 1, 2] and single_template_concept_avg's arithmetic on `raw` (text_embeddings.py:173-183:
                    sum / count per class, then the norm), float64 [3, 32]
    noise_f32       max |float32 run - float64 run| over the unit rows: the noise floor of float32 arithmetic at these dimensions

One thing of the reference is patched at run time: its `utils.LayerNorm` casts the input to float32 (written for fp16
weights), which would put a float32 rounding into the float64 run.  For the float64 run `utils.LayerNorm.forward` is set to
`nn.LayerNorm.forward`; the float32 run uses the reference's class as it is.

    python tests/golden/gen_golden_text.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402  (paths)
import text_ref as R  # noqa: E402

DIMS = dict(context_length=9, vocab_size=40, transformer_width=128, transformer_heads=2, transformer_layers=2, embed_dim=32)
LENGTHS = [2, 3, 4, 5, 6]
COUNTS = [2, 1, 2]
SEED = 77


def grid_state():
    sd = R.seeded_clip_text_state(DIMS["context_length"], DIMS["vocab_size"], DIMS["transformer_width"],
                                  DIMS["transformer_layers"], DIMS["embed_dim"], SEED)
    sd = {k: torch.round(v * 128.0) / 128.0 for k, v in sd.items()}
    assert all(torch.equal(v.half().float(), v) for v in sd.values())
    return sd


def main():
    os.chdir(G.REF)
    sys.path.insert(0, G.REF)
    import _ref_shim
    _ref_shim.install()
    import third_party.zegclip.models.backbones.utils as ref_utils
    from third_party.zegclip.models.backbones.text_encoder import CLIPTextEncoder

    sd = grid_state()
    tokens = R.seeded_tokens(LENGTHS, DIMS["context_length"], DIMS["vocab_size"], SEED + 1)
    assert (tokens[:, 0] == 38).all() and all(tokens[r, n - 1] == 39 for r, n in enumerate(LENGTHS))

    def run(f64):
        keep = ref_utils.LayerNorm.forward
        if f64:
            torch.set_default_dtype(torch.float64)
            ref_utils.LayerNorm.forward = nn.LayerNorm.forward
        try:
            m = CLIPTextEncoder(**DIMS)
            m.load_state_dict({k: (v.double() if f64 else v) for k, v in sd.items()}, strict=True)
            assert all(p.dtype == (torch.float64 if f64 else torch.float32) for p in m.parameters())
            with torch.no_grad():
                out = m(tokens)
            assert out.dtype == (torch.float64 if f64 else torch.float32)
            return out, {k: tuple(v.shape) for k, v in m.state_dict().items()}
        finally:
            ref_utils.LayerNorm.forward = keep
            torch.set_default_dtype(torch.float32)

    raw, shapes = run(True)
    raw32, _ = run(False)
    assert shapes == {k: tuple(v.shape) for k, v in sd.items()}
    out = raw / raw.norm(dim=-1, keepdim=True)
    out32 = raw32 / raw32.norm(dim=-1, keepdim=True)
    noise = (out32.double() - out).abs().max().item()
    # single_template_concept_avg's arithmetic (text_embeddings.py:173-183) on the float64 rows
    avg, o = [], 0
    for c in COUNTS:
        avg.append(torch.sum(raw[o:o + c], dim=0) / c)
        o += c
    avg = torch.stack(avg, dim=0)
    avg = avg / avg.norm(dim=-1, keepdim=True)
    mine = R.encode(sd, tokens)
    print(f"[text] float32 run: {noise:.2e} from the float64 run on unit rows; tests/text_ref.py: "
          f"{(mine - out).abs().max().item():.2e} from the float64 run, concept average "
          f"{(R.concept_avg(sd, tokens, COUNTS) - avg).abs().max().item():.2e}")
    res = dict(dims=np.array(repr(DIMS)), tokens=tokens.numpy(), raw=raw.numpy(), out=out.numpy(),
               counts=np.array(COUNTS, dtype=np.int64), avg=avg.numpy(), noise_f32=np.array(noise))
    for k, v in sd.items():
        res["w/" + k] = v.half().numpy()
    path = os.path.join(HERE, "text_encoder.npz")
    np.savez_compressed(path, **res)
    print(f"    wrote {path} ({os.path.getsize(path) / 1e3:.0f} KB)")
    assert os.path.getsize(path) <= 512 * 1024


if __name__ == "__main__":
    main()
