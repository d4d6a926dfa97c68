#!/usr/bin/env python
"""Train the weights of the GRU user model with torch autograd and write them as helpers.GRUUserModel's .npz.

This is a TOOL, not product code: the comparison route of the device trainer, helpers.fit_gru_user_model (dae_gru_pair_loss: BPTT
kernels in the library).  It is no longer the only way to weights -- main_autoencoder.py --user_model gru --fit_gru trains
on the device -- but it is what tests/test_hip_gru_fit.py holds the device fit against and what tools/gru_fit_bench.py times it
against, and it trains on the CPU where there is no device.

Model and loss: a torch.nn.GRU (one layer, hidden size = embedding size) reads every user's clicks oldest first, x = E[item]
with E fixed; the state u_t after event t predicts event t + 1 by the pairwise ranking loss of helpers.user_pair_loss,

    loss = mean over the valid pairs of softplus(-(u_t . E[items[t + 1]] - u_t . E[negative]))

with the negatives of helpers.sample_negatives (fresh per epoch, seeded).  Padded mini-batches of users, Adam.

    python tools/gru_fit_torch.py --embeddings emb.npy --sessions sessions.npz --out gru.npz [--epochs 5] [--device cpu]
    python tools/gru_fit_torch.py --synthetic 2000x64 --users 1000 --out gru.npz      # seeded embeddings and sessions
    python tools/gru_fit_torch.py --cell lstm --embeddings emb.npy --sessions sessions.npz --out lstm.npz

--cell lstm / --cell rnn train a torch.nn.LSTM / torch.nn.RNN (tanh) the same way and write helpers.LSTMUserModel's /
helpers.RNNUserModel's .npz: the comparison route of helpers.fit_lstm_user_model / helpers.fit_rnn_user_model (dae_lstm_pair_loss,
dae_rnn_pair_loss), as the default is of the GRU's -- what tests/test_hip_lstm_rnn_fit.py holds the device fits against and
tools/rnn_fit_bench.py times them against.  The default, --cell gru, is unchanged.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fit(E, indptr, items, *, epochs=5, batch_users=256, n_neg=4, lr=1e-2, seed=0, max_events=50, device="cpu", log=print, cell="gru"):
    """Returns (torch.nn.GRU -- or, by ``cell``, torch.nn.LSTM / torch.nn.RNN --, loss per pair of every epoch)."""
    import torch
    from dae_rnn_news_recommendation_amd import helpers
    torch.manual_seed(seed)
    dev = torch.device(device)
    E_t = torch.as_tensor(np.asarray(E, dtype=np.float32)).to(dev)
    Na, D = E_t.shape
    indptr, items = helpers.trim_histories((np.asarray(indptr, np.int64), np.asarray(items, np.int64)), max_events)
    lens = np.diff(indptr)
    users = np.flatnonzero(lens >= 2)
    gru = {"gru": torch.nn.GRU, "lstm": torch.nn.LSTM, "rnn": torch.nn.RNN}[cell](D, D, batch_first=True).to(dev)
    opt = torch.optim.Adam(gru.parameters(), lr=lr)
    rng = np.random.default_rng(seed)
    history = []
    for ep in range(epochs):
        neg = helpers.sample_negatives(indptr, items, Na, n_neg, seed * 1000003 + ep)      # [events x n_neg], -1 = no pair
        total, pairs = 0.0, 0
        perm = rng.permutation(users)
        for b0 in range(0, perm.size, batch_users):
            ub = perm[b0:b0 + batch_users]
            T = int(lens[ub].max())
            it = np.zeros((ub.size, T), np.int64)
            ng = np.full((ub.size, T, n_neg), -1, np.int64)
            for r, u in enumerate(ub):
                a, b = indptr[u], indptr[u + 1]
                it[r, :b - a] = items[a:b]
                ng[r, :b - a] = neg[a:b]
            it_t, ng_t = torch.from_numpy(it).to(dev), torch.from_numpy(ng).to(dev)
            states, _ = gru(E_t[it_t[:, :-1]])                                              # u_t for t = 0 .. T - 2
            pos, ngn = E_t[it_t[:, 1:]], ng_t[:, 1:]                                        # event t + 1 and its negatives
            valid = ngn >= 0
            x = (states * pos).sum(-1, keepdim=True) - torch.einsum("uth,utnh->utn", states, E_t[ngn.clamp(min=0)])
            n = int(valid.sum())
            if n == 0:
                continue
            loss = (torch.nn.functional.softplus(-x) * valid).sum() / n
            opt.zero_grad()
            loss.backward()
            opt.step()
            total += float(loss.detach()) * n
            pairs += n
        history.append(total / max(pairs, 1))
        log("epoch %d: loss per pair %.4f (%d pairs)" % (ep + 1, history[-1], pairs))
    return gru, np.asarray(history)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--embeddings", default="", help=".npy [articles x H]")
    p.add_argument("--sessions", default="", help=".npz with indptr and items (main_autoencoder.py --sessions)")
    p.add_argument("--synthetic", default="", help="ARTICLESxH: seeded class-centred embeddings and synthetic sessions instead of files")
    p.add_argument("--users", type=int, default=1000, help="users of --synthetic")
    p.add_argument("--out", required=True)
    p.add_argument("--epochs", type=int, default=5)
    p.add_argument("--batch_users", type=int, default=256)
    p.add_argument("--n_neg", type=int, default=4)
    p.add_argument("--lr", type=float, default=1e-2)
    p.add_argument("--max_events", type=int, default=50)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cpu")
    p.add_argument("--cell", default="gru", choices=["gru", "lstm", "rnn"], help="the recurrent cell: torch.nn.GRU (default), LSTM or RNN (tanh)")
    a = p.parse_args(argv)
    from dae_rnn_news_recommendation_amd import helpers
    if a.synthetic:
        from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
        Na, H = (int(v) for v in a.synthetic.lower().split("x"))
        rng = np.random.default_rng(a.seed)
        labels = rng.integers(0, max(Na // 100, 2), Na)
        centres = rng.standard_normal((int(labels.max()) + 1, H))
        E = (centres[labels] + 0.5 * rng.standard_normal((Na, H))).astype(np.float32)
        indptr, items = synthetic_sessions(a.users, labels, mean_len=12, seed=a.seed)
    else:
        assert a.embeddings and a.sessions, "--embeddings and --sessions, or --synthetic"
        E = np.load(a.embeddings)
        with np.load(a.sessions) as f:
            indptr, items = np.asarray(f["indptr"], np.int64), np.asarray(f["items"], np.int64)
    gru, history = fit(E, indptr, items, epochs=a.epochs, batch_users=a.batch_users, n_neg=a.n_neg, lr=a.lr, seed=a.seed,
                       max_events=a.max_events, device=a.device, cell=a.cell)
    {"gru": helpers.GRUUserModel, "lstm": helpers.LSTMUserModel, "rnn": helpers.RNNUserModel}[a.cell].from_torch(gru).save(a.out)
    print("wrote %s (H = %d, %d epochs, loss per pair %.4f -> %.4f)" % (a.out, E.shape[1], history.size, history[0], history[-1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
