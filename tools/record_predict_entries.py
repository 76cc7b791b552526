"""Records the library entries a plain `predict` calls (tests/golden/spec_no_draft_entries.json), which
tests/test_spec_decode_gpu.py::test_without_a_draft_the_entries_called_are_the_parents pins: speculative decoding is opt-in, and
without `draft=` the route must call what it called before the feature existed -- the same entries, the same number of times, in the
same order.

    python tools/record_predict_entries.py CHECKOUT [OUT.json]

CHECKOUT is the root of a BUILT checkout of this project; the package is imported from there and from nowhere else, so the golden is
taken with a checkout of the commit before the feature (07a8902, "GEMM family: ..."):

    git worktree add ../parent 07a8902 && make -C ../parent/omr_a2s_multimodal_transformer_amd/csrc
    python tools/record_predict_entries.py ../parent tests/golden/spec_no_draft_entries.json

The case (model, inputs, batch size) is tests/spec_refs.py's PREDICT_CASE, built by its build_predict_case from the package of CHECKOUT.
Needs a GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main() -> None:
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    checkout = os.path.abspath(sys.argv[1])
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
    sys.path.insert(0, checkout)
    import torch
    import omr_a2s_multimodal_transformer_amd as pkg
    assert os.path.dirname(os.path.dirname(os.path.abspath(pkg.__file__))) == checkout, pkg.__file__
    import spec_refs
    with torch.no_grad():
        m, xs = spec_refs.build_predict_case()
        words = []
        entries = spec_refs.record_entries(lambda: words.extend(m.predict(xs, batch_size=spec_refs.PREDICT_CASE["batch_size"])))
    out = {"case": spec_refs.PREDICT_CASE, "tokens": [len(w) for w in words], "entries": entries}
    text = json.dumps(out, indent=0)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text + "\n")
    print(f"{len(entries)} entries, {len(set(entries))} distinct; tokens per input {out['tokens']}")


if __name__ == "__main__":
    main()
