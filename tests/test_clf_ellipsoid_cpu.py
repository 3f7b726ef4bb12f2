"""The ellipsoid classifier's call surface (BOBE/clf.py:125-166, 221-285, 375-472) and the test restatement it is
measured against (tests/ellipsoid_restatement.py): no GPU is touched."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import ellipsoid_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "reference_signatures.json")) as _fh:
    REF = json.load(_fh)["modules"]["clf"]["functions"]

NAMES = ["train_ellipsoid_classifier", "get_ellipsoid_predict_proba_fn", "train_with_restarts", "train_ellipsoid",
         "train_ellipsoid_multiple_restarts"]


@pytest.mark.parametrize("name", NAMES)
def test_functions_start_with_the_reference_parameters(name):
    from bobe_amd import clf
    fn = getattr(clf, name)
    ours = list(inspect.signature(fn).parameters.values())
    ref = REF[name]["params"]
    fixed = [p for p in ref if p["kind"] not in ("var_positional", "var_keyword")]
    ours_fixed = [p for p in ours if p.kind not in (p.VAR_POSITIONAL, p.VAR_KEYWORD)]
    assert [p.name for p in ours_fixed[:len(fixed)]] == [p["name"] for p in fixed]
    for r, o in zip(fixed, ours_fixed):
        assert o.kind == inspect.Parameter.POSITIONAL_OR_KEYWORD
        if r["default"] is None:
            continue
        if r["default"] == "{}":                       # (a mutable {} default becomes None)
            assert o.default is None, (name, r["name"])
        else:
            assert o.default == eval(r["default"]), (name, r["name"], o.default)       # noqa: S307 - literals only
    for extra in ours_fixed[len(fixed):]:
        assert extra.default is not inspect.Parameter.empty
    if any(p["kind"] == "var_keyword" for p in ref):
        assert any(p.kind == inspect.Parameter.VAR_KEYWORD for p in ours)


def test_ellipsoid_classifier_fields_and_defaults():
    """clf.py:377-389: the module's fields, in order, with their defaults; an unknown setting is a TypeError, d beyond the
    library's limit a ValueError naming it."""
    from bobe_amd.clf import EllipsoidClassifier
    params = list(inspect.signature(EllipsoidClassifier).parameters.values())
    want = [("d", None), ("mu", None), ("init_scale", 0.1), ("lr", 1e-2), ("weight_decay", 1e-4), ("n_epochs", 1000),
            ("batch_size", 64), ("patience", 25), ("n_restarts", 2), ("val_frac", 0.1), ("seed_offset", 0),
            ("split_seed", 42)]
    assert [p.name for p in params] == [w[0] for w in want]
    for p, (_, dflt) in zip(params, want):
        if dflt is None:
            assert p.default is inspect.Parameter.empty
        else:
            assert p.default == dflt and type(p.default) is type(dflt)
    m = EllipsoidClassifier(d=3, mu=np.full(3, 0.2))
    assert m.n_tril == 6 and m.batch_size == 64 and m.n_restarts == 2
    p0 = m.init(123)["params"]
    assert np.array_equal(p0["flat_L"], np.random.default_rng(123).normal(0.0, 0.1, size=6))
    assert p0["alpha"] == 1.0 and p0["beta"] == 0.0
    with pytest.raises(TypeError):
        EllipsoidClassifier(d=3, mu=np.zeros(3), hidden_dims=(8,))
    with pytest.raises(ValueError, match="32"):
        EllipsoidClassifier(d=33, mu=np.zeros(33))


def test_permutation_table_follows_the_reference_batches():
    """clf.py:446-452: RandomState(seed), one permutation per epoch, the tail dropped; N < B is one batch of all rows."""
    from bobe_amd.clf import ellipsoid_permutations
    for n, b in ((40, 64), (300, 64), (1000, 64), (128, 64)):
        tab = ellipsoid_permutations(77, n, 5, b)
        rs = np.random.RandomState(77)
        steps = max(1, n // b)
        for e in range(5):
            perm = rs.permutation(n)
            want = np.concatenate([perm[i * b:(i + 1) * b] for i in range(steps)])
            assert tab.dtype == np.int32 and np.array_equal(tab[e], want)


def test_restart_choice_is_the_first_smallest_formatted_loss():
    from bobe_amd.clf import _select_best
    runs = [("a", {"train_loss": "1.23e-01"}), ("b", {"train_loss": "1.23e-01"}), ("c", {"train_loss": "1.24e-01"})]
    assert _select_best(runs)[0] == "a"
    assert _select_best(runs[::-1])[0] == "b"
    assert _select_best([("a", {"train_loss": "2.00e-01"}), ("b", {"train_loss": "1.99e-01"})])[0] == "b"


def _problem(d, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, d))
    mu = np.full(d, 0.5)
    y = (np.sum((x - mu) ** 2, axis=1) < 0.08 * d).astype(np.float64)
    start = {"flat_L": rng.normal(0, 0.3, size=d * (d + 1) // 2), "alpha": 1.3, "beta": 0.4}
    return x, y, mu, start


@pytest.mark.parametrize("d", [1, 3, 6])
def test_restatement_gradient_against_autograd_and_central_differences(d):
    x, y, mu, p = _problem(d, 50, d)
    fl = torch.tensor(p["flat_L"], requires_grad=True)
    al = torch.tensor(p["alpha"], dtype=torch.float64, requires_grad=True)
    be = torch.tensor(p["beta"], dtype=torch.float64, requires_grad=True)
    R.bce(R.logits(fl, al, be, mu, x)[0], y).backward()
    gf, ga, gb = R.analytic_grad(p["flat_L"], p["alpha"], p["beta"], mu, x, y)
    assert np.allclose(gf, fl.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert ga == pytest.approx(float(al.grad), rel=1e-12) and gb == pytest.approx(float(be.grad), rel=1e-12)

    def loss(theta):
        t = len(theta) - 2
        return float(R.bce(R.logits(theta[:t], theta[t], theta[t + 1], mu, x)[0], y))
    theta = np.concatenate([p["flat_L"], [p["alpha"], p["beta"]]])
    fd = np.empty_like(theta)
    for i in range(len(theta)):
        e = np.zeros_like(theta)
        e[i] = 1e-6
        fd[i] = (loss(theta + e) - loss(theta - e)) / 2e-6
    assert np.allclose(np.concatenate([gf, [ga, gb]]), fd, rtol=1e-6, atol=1e-9)


def test_restatement_logit_forms_agree():
    """The L L^T einsum of the reference and |L^T diff|^2 (the library's form) are the same function."""
    x, _, mu, p = _problem(5, 200, 9)
    lg, md2 = R.logits(p["flat_L"], p["alpha"], p["beta"], mu, x)
    L = R.unpack_L(p["flat_L"], 5).numpy()
    u = (x - mu) @ L
    assert np.allclose(md2.numpy(), np.sum(u * u, axis=1), rtol=1e-13)
    assert np.allclose(lg.numpy(), -p["alpha"] * np.sum(u * u, axis=1) + p["beta"], rtol=1e-13, atol=1e-13)


def test_restatement_adamw_is_optax_adamw():
    """Three AdamW steps of the restatement's optimiser (torch.optim.AdamW) against optax.adamw written out:
    scale_by_adam (bias correction with count from 1, eps_root 0) -> add_decayed_weights -> scale_by_learning_rate."""
    x, y, mu, p = _problem(3, 64, 4)
    lr, wd = 1e-2, 1e-4
    fl = torch.tensor(p["flat_L"], requires_grad=True)
    al = torch.tensor(p["alpha"], dtype=torch.float64, requires_grad=True)
    be = torch.tensor(p["beta"], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.AdamW([fl, al, be], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    theta = np.concatenate([p["flat_L"], [p["alpha"], p["beta"]]])
    m, v = np.zeros_like(theta), np.zeros_like(theta)
    for count in (1, 2, 3):
        idx = np.arange(count * 10, count * 10 + 30)
        opt.zero_grad()
        R.bce(R.logits(fl, al, be, mu, x[idx])[0], y[idx]).backward()
        opt.step()
        t = len(theta) - 2
        gf, ga, gb = R.analytic_grad(theta[:t], theta[t], theta[t + 1], mu, x[idx], y[idx])
        g = np.concatenate([gf, [ga, gb]])
        m = (1 - 0.9) * g + 0.9 * m
        v = (1 - 0.999) * g ** 2 + 0.999 * v
        mh, vh = m / (1 - 0.9 ** count), v / (1 - 0.999 ** count)
        upd = mh / (np.sqrt(vh + 0.0) + 1e-8) + wd * theta
        theta = theta + (-lr) * upd
        got = np.concatenate([fl.detach().numpy(), [al.item(), be.item()]])
        assert np.allclose(got, theta, rtol=1e-12, atol=1e-14), count
