"""Records the loss that tests/test_ragged_training_gpu.py test 12 pins (tests/golden/ragged_dense_loss.json): the dense route (1-D xl)
of the small test model at B = 2, 32 x 96, T = 12, in fp32 and bf16, as the hex bits of the fp32 loss.

    python tools/record_dense_loss.py CHECKOUT [OUT.json]

CHECKOUT is the root of a BUILT checkout of this project; the package is imported from there and from nowhere else, so the golden
of the commit before the ragged route is taken with a checkout of that commit (f3bd580, "Conv kernels: exact-sum tests through the
persistent tile loops"):

    git worktree add ../parent f3bd580 && make -C ../parent/omr_a2s_multimodal_transformer_amd/csrc
    python tools/record_dense_loss.py ../parent tests/golden/ragged_dense_loss.json

Run against this tree it prints the bits the test computes.  The model, seed and batch are those of the test's make_model /
synthetic_unimodal_batch(seed=3); needs a GPU."""
import json
import os
import sys


def main() -> None:
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, root)
    import torch
    import omr_a2s_multimodal_transformer_amd as pkg
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    assert os.path.abspath(pkg.__file__).startswith(root + os.sep), f"imported {pkg.__file__}, not the package under {root}"
    V, T, D, LAYERS = 30, 12, 128, 2
    out = {}
    for dtype in ("fp32", "bf16"):
        w2i, i2w = syn.make_vocab(V)
        cfg = ModelConfig(d_model=D, ff_dim=D, num_layers=LAYERS, dropout=0.0, encoder_dropout=0.0, compute_dtype=dtype)
        m = Transformer(64, 96, T + 4, w2i, i2w, config=cfg)
        m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(V, D, D, LAYERS), 23), strict=False)
        m.flatten_parameters()
        m.teacher_forcing_prob = 0.0
        m.eval()
        x, xl, y_in, y_out = syn.synthetic_unimodal_batch(2, 32, 96, T, V, w2i["<sos>"], w2i["<eos>"], seed=3)
        with torch.no_grad():
            loss = m.compute_loss(m(x.to("cuda:0"), xl, y_in), y_out.to("cuda:0")).float()
        out[dtype] = format(int(loss.cpu().view(torch.int32)) & 0xFFFFFFFF, "08x")
        print(dtype, repr(float(loss)), out[dtype], flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as fh:
            json.dump(out, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
