"""CPU tests of the optimiser's references (tests/ctc_optim_ref.py): adam_ref in
float64 is torch's clip_grad_norm_ + optim.Adam; every mutation of it -- the
mistakes an Adam kernel makes -- moves some tensor far past the GPU bound on
the generated gradients; and train_ctc's bookkeeping, with a stub trainer."""
import copy

import pytest
import torch

import ctc_optim_ref as O
import ctc_ref as R

V = 512


@pytest.mark.parametrize("run", list(O.RUNS))
def test_adam_ref_is_torch_adam(run):
    """Three steps on a float64 module: clip_grad_norm_ then Adam.step, against adam_ref, to 1e-12."""
    hyper = dict(O.HYPER, **O.RUNS[run])
    grads, _ = O.gradients(V)
    grads = grads[:3]
    m = copy.deepcopy(R.model(V)).double()
    opt = torch.optim.Adam(m.parameters(), lr=hyper["lr"], betas=hyper["betas"], eps=hyper["eps"],
                           weight_decay=hyper["weight_decay"])
    named = dict(m.named_parameters())
    norms = []
    for g in grads:
        for k, gk in O.split(g.double(), V).items():
            named[k].grad = gk.clone()
        if hyper["max_norm"] > 0:
            norms.append(torch.nn.utils.clip_grad_norm_(m.parameters(), hyper["max_norm"]).detach().clone())
        else:
            norms.append(g.double().norm())
        opt.step()
    p, mm, vv = O.adam_ref(O.p0(V), grads, norms, torch.float64, **hyper)
    state = {k: opt.state[named[k]] for k in named}
    got_p = O.flat_weights(m, V, torch.float64)
    got_m = torch.cat([state[k]["exp_avg"].reshape(-1) for k, _ in O.spec(V)])
    got_v = torch.cat([state[k]["exp_avg_sq"].reshape(-1) for k, _ in O.spec(V)])
    # the weights (|p| up to about 16) as the absolute difference, the moments relative to each tensor's largest value
    for what, got, ref in (("p", got_p, p), ("m", got_m, mm), ("v", got_v, vv)):
        e = {k: float((a - b).abs().max()) for (k, a), b in zip(O.split(got, V).items(), O.split(ref, V).values())} \
            if what == "p" else O.errors(got, ref, None, V)
        worst = max(e.values())
        print(f"{run} {what}: worst {worst:.3g}")
        assert worst <= 1e-12, (what, e)


def test_generated_norms_straddle_the_clip():
    _, norms = O.gradients(V)
    assert [round(float(n), 3) for n in norms] == list(O.NORMS)
    assert sum(float(n) > O.HYPER["max_norm"] for n in norms) == 3
    g = O.gradients(V)[0][0]
    assert 0.005 < float((g == 0).float().mean()) < 0.02


@pytest.mark.parametrize("mutation", O.MUTATIONS)
def test_mutations_exceed_the_bound(mutation):
    """Each mutation moves at least one tensor (weights or moments) by >= 100 times that tensor's bound."""
    c = O.opt_case(V, "weight_decay" if mutation == "decoupled_wd" else "plain")
    e = c.measure(O.adam_ref(c.p0, c.grads, c.norms, torch.float64, mutation=mutation, **c.hyper))
    ratios = {(what, k): e[what][k] / c.bound(what, k) for what in e for k in e[what]}
    (what, k), worst = max(ratios.items(), key=lambda kv: kv[1])
    print(f"{mutation}: worst {what} {k} at {worst:.3g} x its bound (K_OPT = {O.K_OPT})")
    assert worst >= 100.0


# ---- train_ctc's bookkeeping -------------------------------------------------------
class StubTrainer:
    """step / val_loss return scripted losses; the state dict records the epoch."""

    def __init__(self, train, val):
        self.train, self.val, self.epoch, self.i, self.calls = train, val, 0, 0, []

    def step(self, feats, labels, fl, ll):
        self.calls.append(("step", feats))
        x = self.train[self.epoch][self.i]
        self.i += 1
        return torch.tensor(x)

    def val_loss(self, feats, labels, fl, ll):
        self.calls.append(("val", feats))
        if self.i:                       # the first validation batch of the epoch
            self.i = 0
            self.epoch += 1
        return torch.tensor(self.val[self.epoch - 1])

    def state_dict(self):
        return {"epoch": self.epoch}


def test_train_ctc_bookkeeping():
    import wakeword
    train_loader = [("a", 0, 0, 0), ("b", 0, 0, 0)]
    val_loader = [("v", 0, 0, 0)]
    train = [[4.0, 2.0], [3.0, 1.0], [1.0, 1.0], [0.5, 0.5], [9.0, 9.0], [9.0, 9.0]]
    val = [5.0, 3.0, 3.5, 3.0, 4.0, 1.0]
    stub = StubTrainer(train, val)
    tr, tl, vl, best = wakeword.train_ctc(train_loader, val_loader, vocab=V, num_epochs=6, patience=3, trainer=stub)
    assert tr is stub
    assert tl == [3.0, 2.0, 1.0, 0.5, 9.0]            # epoch means; stopped after 3 epochs without improvement
    assert vl == [5.0, 3.0, 3.5, 3.0, 4.0]
    assert best == {"epoch": 2}                       # a tie (epoch 4's 3.0) is no improvement
    assert [c[0] for c in stub.calls[:3]] == ["step", "step", "val"]
    # patience not reached: every epoch runs, and the last best is kept
    stub = StubTrainer(train, val)
    _, tl, vl, best = wakeword.train_ctc(train_loader, val_loader, vocab=V, num_epochs=6, patience=4, trainer=stub)
    assert len(tl) == 6 and vl == val and best == {"epoch": 6}
    with pytest.raises(ValueError):
        wakeword.train_ctc(train_loader, val_loader, vocab=V, trainer=stub, lr=1e-2)
