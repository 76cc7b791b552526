"""Host restatements for the speculative-decoding tests: the acceptance rule of omr_spec_accept in numpy, and a fake pair of
models that replays fixed sequences through the callbacks of evaluation.decode_spec."""
import numpy as np


def accept(tokens, picks, top1, state, k, eos, max_out):
    """omr_spec_accept on host arrays.  tokens / picks int64 [B][k+1], top1 fp32 [B][k+1]; state: dict of pos, out_len, done,
    accepted (int32 [B]), totals (int64 [2]), first, prev (int64 [B]), out_tokens (int64 [B][max_out]), out_top1 (fp32) --
    updated in place.  Per live slot: j = leading proposals equal to the pick before them; picks[0..j] are appended, cut after the
    first <eos> and at max_out (either sets done)."""
    B = tokens.shape[0]
    for b in range(B):
        if state["done"][b]:
            state["accepted"][b] = 0
            continue
        j = 0
        while j < k and tokens[b, j + 1] == picks[b, j]:
            j += 1
        n, done = j + 1, 0
        for i in range(n):
            if picks[b, i] == eos:
                n, done = i + 1, 1
                break
        length = int(state["out_len"][b])
        room = max_out - length
        if n >= room:
            n, done = room, 1
        state["out_tokens"][b, length:length + n] = picks[b, :n]
        state["out_top1"][b, length:length + n] = top1[b, :n]
        if n > 0:
            state["prev"][b] = picks[b, n - 2] if n >= 2 else state["first"][b]
            state["first"][b] = picks[b, n - 1]
            state["out_len"][b] = length + n
            state["pos"][b] += n
        state["done"][b] = done
        state["accepted"][b] = j
        state["totals"][0] += k
        state["totals"][1] += j


def new_state(B, max_out, first, sos, eos):
    """The state after position 0: one token per slot."""
    st = dict(pos=np.ones(B, np.int32), out_len=np.ones(B, np.int32), done=np.zeros(B, np.int32), accepted=np.zeros(B, np.int32),
              totals=np.zeros(2, np.int64), first=np.array(first, np.int64), prev=np.full(B, sos, np.int64),
              out_tokens=np.zeros((B, max_out), np.int64), out_top1=np.zeros((B, max_out), np.float32))
    st["out_tokens"][:, 0] = first
    st["done"][:] = [int(t == eos or max_out <= 1) for t in first]
    return st


class Replay:
    """A target that replays truth[b] (the token of every position, whatever it is fed -- as long as it is fed its own prefix, which
    is what a correct driver does) and a draft that proposes guess[b][t] for position t.  cycles / plain are the callbacks of
    evaluation.decode_spec; `value` of a token at position t of row b is 1000 * b + t, so a misplaced token shows."""

    def __init__(self, truth, guess, k, eos, budget, sos=2):
        self.truth, self.guess, self.k, self.eos, self.budget = truth, guess, k, eos, budget
        B = len(truth)
        self.state = new_state(B, budget, [seq[0] for seq in truth], sos, eos)
        self.state["out_top1"][:, 0] = [1000.0 * b for b in range(B)]
        self.lens = [1] * B
        self.calls = []

    def first(self):
        return [seq[0] for seq in self.truth], [1000.0 * b for b in range(len(self.truth))]

    def _truth(self, b, t):
        return self.truth[b][t] if t < len(self.truth[b]) else 7

    def _guess(self, b, t):
        return self.guess[b][t] if t < len(self.guess[b]) else 9

    def cycles(self, n, t_max):
        st, B, R = self.state, len(self.truth), self.k + 1
        self.calls.append(("cycles", n, t_max))
        assert t_max + n * R <= self.budget, "the driver enqueued cycles past the budget"
        assert t_max >= max(int(st["pos"][b]) for b in range(B) if not st["done"][b]), "t_max is not an upper bound of the live positions"
        for _ in range(n):
            tokens = np.zeros((B, R), np.int64)
            picks = np.zeros((B, R), np.int64)
            top1 = np.zeros((B, R), np.float32)
            for b in range(B):
                p = int(st["pos"][b])
                assert st["done"][b] or st["first"][b] == self._truth(b, p - 1)
                tokens[b, 0] = st["first"][b]
                for r in range(1, R):
                    tokens[b, r] = self._guess(b, p + r - 1)
                for r in range(R):           # the pick of position p + r is the truth only while the row was fed its own prefix
                    fed_own = all(tokens[b, i] == self._truth(b, p + i - 1) for i in range(1, r + 1))
                    picks[b, r] = self._truth(b, p + r) if fed_own else 5
                    top1[b, r] = 1000.0 * b + p + r
            accept(tokens, picks, top1, st, self.k, self.eos, self.budget)
        new_t, new_v = [], []
        for b in range(B):
            n_b = int(st["out_len"][b])
            new_t.append(st["out_tokens"][b, self.lens[b]:n_b].tolist())
            new_v.append(st["out_top1"][b, self.lens[b]:n_b].tolist())
            self.lens[b] = n_b
        return new_t, new_v

    def plain(self, n, pos):
        self.calls.append(("plain", n, list(pos)))
        assert max(pos) + n <= self.budget
        toks = [[self._truth(b, pos[b] + s) for b in range(len(pos))] for s in range(n)]
        vals = [[1000.0 * b + pos[b] + s for b in range(len(pos))] for s in range(n)]
        return toks, vals


# ---- the no-draft case whose library entries tests/golden/spec_no_draft_entries.json records (tools/record_predict_entries.py)
PREDICT_CASE = dict(V=97, max_seq=300, sizes=[(32, 280), (32, 1200), (32, 512)], seed=61, input_seed=900, batch_size=4)


def build_predict_case(device="cuda:0"):
    """-> (model, inputs) of PREDICT_CASE, from whichever checkout of the package is first on sys.path: a 2-layer d = 128 fp32
    Transformer with seeded weights and <eos> suppressed (every row runs max_seq positions, so the number of host calls does not
    hang on a token), and three inputs of 70, 300 and 128 memory keys."""
    import torch
    from omr_a2s_multimodal_transformer_amd import synthetic as syn
    from omr_a2s_multimodal_transformer_amd.config import ModelConfig
    from omr_a2s_multimodal_transformer_amd.model import Transformer
    c = PREDICT_CASE
    cfg = ModelConfig(d_model=128, nhead=4, ff_dim=256, num_layers=2, compute_dtype="fp32", dropout=0.0, encoder_dropout=0.0)
    w2i, i2w = syn.make_vocab(c["V"])
    m = Transformer(64, 1600, c["max_seq"], w2i, i2w, config=cfg)
    m.load_state_dict(syn.seeded_state_dict(syn.transformer_shapes(c["V"], 128, 256, 2), c["seed"]), strict=False)
    m.flatten_parameters()
    m.eval()
    m.decoder.out_layer.bias.omr_phys[w2i["<eos>"]] = -1e4
    xs = []
    for i, s in enumerate(c["sizes"]):
        g = torch.Generator().manual_seed(c["input_seed"] + i)
        xs.append(torch.rand((1, 1) + tuple(s), generator=g).to(device))
    return m, xs


def record_entries(fn):
    """Runs fn() and returns the names of the library entries it called (lib().call / lib().query), in call order."""
    from omr_a2s_multimodal_transformer_amd._lib import lib
    fns, called, saved = lib().fns, [], dict(lib().fns)

    def recorder(name, f):
        def call(*a):
            called.append(name)
            return f(*a)
        return call

    try:
        for name in saved:
            fns[name] = recorder(name, saved[name])
        fn()
    finally:
        fns.update(saved)
    return called
