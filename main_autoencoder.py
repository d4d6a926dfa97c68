#!/usr/bin/env python3
"""Command-line trainer with the flag surface of the reference's ``main_autoencoder.py`` (:27-74) on the
MI355X-native estimator.

Kept: flag names, defaults, choices and the validation asserts (:94-109), ``main_dir`` defaulting to
``model_name`` (:111), the fit -> transform(decay-compensated) sequence (:277-290), parameter.txt, the saved
artefact names under results/<algo>/<main_dir>/data/.  Not kept (out of the hot path): the parquet /
jieba tokenising and the matplotlib ROC plots -- the UCI dataset blob is absent from the
reference checkout (.MISSING_LARGE_BLOBS:2), so data comes from ``--data <matrix.npz> [--labels <labels.npy>]``
(scipy CSR / dense .npy) or from the seeded synthetic generator (default).  With ``--vectorize`` the file is a raw count
matrix and the CountVectorizer pruning / TfidfTransformer steps (:206-240) run on the device.

examples:
  python main_autoencoder.py --model_name demo --num_epochs 5 --verbose --verbose_step 1
  python main_autoencoder.py --model_name uci --data X.npz --labels y.npy --triplet_strategy batch_hard
  python main_autoencoder.py --model_name bow --data counts.npz --vectorize --validation --min_df 0.001 --max_features 10000
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --rank_metrics --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --rank_metrics --max_age 48 --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --fit_user_model --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --every_click --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --rec_dedup 0.9 --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --rec_mmr 0.7 --rec_max_per_label 3 --similarity False
  python main_autoencoder.py --model_name topics --cluster 40 --validation --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --ann_clusters 64 --ann_probe 8 --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --covisit --covisit_window 3 --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --als --als_factors 64 --als_iterations 15 --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --words --words_idf --rank_metrics --similarity False
  python main_autoencoder.py --model_name rec --sessions synthetic --recommend 10 --every_click --user_model gru --fit_gru --gru_validation 0.2 --similarity False
"""
import argparse
import os
import sys

import numpy as np
from scipy import sparse

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def str2bool(v):
    return str(v).lower() in ("1", "true", "t", "yes", "y")


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    b = dict(type=str2bool, nargs="?", const=True)
    # Global configuration (reference :27-35)
    p.add_argument("--verbose", default=False, **b)
    p.add_argument("--verbose_step", type=int, default=5)
    p.add_argument("--encode_full", default=False, **b)
    p.add_argument("--validation", default=False, **b)
    p.add_argument("--input_format", default="binary", choices=["binary", "tfidf"])
    p.add_argument("--label", default="category_publish_name", choices=["category_publish_name", "story"])
    p.add_argument("--save_tsv", default=False, **b)
    p.add_argument("--train_row", type=int, default=8000)
    p.add_argument("--validate_row", type=int, default=2000)
    # Count-vectorizer parameters (:47-50); only max_features matters for synthetic data; with --vectorize all three prune --data
    p.add_argument("--restore_previous_data", default=False, **b)
    p.add_argument("--min_df", type=float, default=0)
    p.add_argument("--max_df", type=float, default=0.99)
    p.add_argument("--max_features", type=int, default=10000)
    # Autoencoder parameters (:56-74)
    p.add_argument("--model_name", default="")
    p.add_argument("--restore_previous_model", default=False, **b)
    p.add_argument("--seed", type=int, default=-1)
    p.add_argument("--compress_factor", type=int, default=20)
    p.add_argument("--corr_type", default="masking", choices=["masking", "salt_and_pepper", "decay", "none"])
    p.add_argument("--corr_frac", type=float, default=0.3)
    p.add_argument("--xavier_init", type=int, default=1)
    p.add_argument("--enc_act_func", default="sigmoid", choices=["sigmoid", "tanh"])
    p.add_argument("--dec_act_func", default="sigmoid", choices=["sigmoid", "tanh", "none"])
    p.add_argument("--main_dir", default="")
    p.add_argument("--loss_func", default="cross_entropy", choices=["mean_squared", "cross_entropy", "cosine_proximity"])
    p.add_argument("--opt", default="gradient_descent", choices=["gradient_descent", "ada_grad", "momentum"])
    p.add_argument("--learning_rate", type=float, default=0.1)
    p.add_argument("--momentum", type=float, default=0.5)
    p.add_argument("--num_epochs", type=int, default=50)
    p.add_argument("--batch_size", type=float, default=0.1)
    p.add_argument("--alpha", type=float, default=1)
    p.add_argument("--triplet_strategy", default="batch_all", choices=["batch_all", "batch_hard", "none"])
    # MI355X-side additions
    p.add_argument("--precision", default="auto", choices=["auto", "f16x2h", "f16x2d", "bf16x3", "fp32", "f16x3", "f16x2", "bf16", "f16"],
                   help="auto (default): per triplet strategy the cheapest mode measured to hold the reference's loss curve within 1e-4 over 100 steps -- batch_all "
                        "/ batch_hard f16x2h, none f16x2d (fp16 MFMA operand images; W and the operands the strategy is sensitive to as hi + lo); bf16x3: split-bf16, "
                        "hi + lo images of every operand; fp32: exact-fp32 MFMA; f16x3: every operand hi + lo fp16; f16x2 (W alone hi + lo) holds 20 steps, not 100; "
                        "bf16 / f16 (single images) are faster still and outside the gate")
    p.add_argument("--rng", default="numpy", choices=["numpy", "philox"])
    p.add_argument("--data", default="", help="scipy-sparse .npz or dense .npy feature matrix (rows = articles)")
    p.add_argument("--labels", default="", help=".npy label vector aligned with --data")
    p.add_argument("--vectorize", default=False, **b,
                   help="--data is a RAW count matrix (scipy .npz): on the device, the first train_row rows fit the vocabulary (--min_df, "
                        "--max_df, --max_features: CountVectorizer's rule) and the idf; the validation rows go through both; "
                        "--input_format picks the binary or the tf-idf matrix for training.  --min_df / --max_df are parsed as floats in "
                        "[0, 1] (the reference's flags), so only shares of the train rows are accepted here; absolute counts are taken by "
                        "helpers.limit_features.  Saves article_[binary_]count_vectorized, "
                        "article_tfidf_vectorized (and their _validate forms), vocabulary_kept.npy and tfidf_transformer.npz.  Off: "
                        "--data is trained on as it is")
    p.add_argument("--data_parallel", default=False, **b)
    p.add_argument("--similarity", default=True, **b,
                   help="after training: the N x N cosine similarities the reference computes (:307-317), on the device")
    p.add_argument("--top_k", type=int, default=0,
                   help="K > 0: after training, the K most similar train articles of every train (and validation) article, written to "
                        "article_encoded[_validate]_top{K}.npz, with precision@K of the input vectors and of the embedding when labels exist "
                        "(no N x N matrix: works with --similarity False on corpora too large for it)")
    p.add_argument("--dup_threshold", type=float, default=0.0,
                   help="T > 0: after training, every pair of train articles whose embeddings have cosine >= T (near duplicates), written "
                        "to article_encoded_dups.npz with the de-duplication groups (keep the first article of each story), and the "
                        "validation articles against the train corpus to article_encoded_validate_dups.npz; with labels, the share of "
                        "pairs with equal labels (no N x N matrix: works with --similarity False)")
    p.add_argument("--label_stats", default=False, **b,
                   help="after training (needs labels): the related-vs-unrelated AUROC, with a bracket that certifies it, and the box-plot "
                        "numbers of the input vectors and of the embeddings, written to similarity_stats_<name>.json (per-class score "
                        "histograms, no N x N matrix: works with --similarity False)")
    p.add_argument("--sweep_chunk_rows", type=int, default=0,
                   help="rows per chunk of the sweeps of --top_k and --label_stats: 0 (default) sweeps every operand whole, as a dense fp32 "
                        "image below 4 GiB; N > 0 sweeps N rows (rounded up to a multiple of 128) at a time and keeps the bag-of-words / "
                        "tf-idf matrix on the device as CSR (same results; for corpora whose dense image does not fit); -1 picks N so that "
                        "a chunk's image is at most 1 GiB")
    p.add_argument("--sessions", default="",
                   help="click logs for --recommend: an .npz with `indptr` (int64, users + 1), `items` (train article indices, every user's clicks "
                        "oldest first) and optionally `timestamps` (one per click), or the word `synthetic` (seeded logs in which a user reads "
                        "mostly from a few label classes; needs labels)")
    p.add_argument("--recommend", type=int, default=0,
                   help="K > 0 (needs --sessions): after training, hold out every user's last click, build decayed user states from the rest "
                        "on the train embeddings, recommend K unseen articles per user to article_encoded_recommend{K}.npz, and print hit@K / "
                        "MRR / nDCG beside a most-clicked-unseen popularity baseline (no users x articles matrix: works with --similarity False)")
    p.add_argument("--rec_dedup", type=float, default=None,
                   help="T (only with --recommend K): ALSO de-duplicated lists -- per user --rec_dedup_pool unseen candidates are "
                        "retrieved and walked best first, skipping an article whose cosine similarity to one already selected is at "
                        "least T (helpers.recommend(dedup_threshold=T)); prints hit@K / MRR / nDCG of those lists and the mean number of "
                        "duplicate pairs per list before and after, and saves article_encoded_recommend{K}_dedup.npz.  The other "
                        "output and files stay what they are")
    p.add_argument("--rec_dedup_pool", type=int, default=0,
                   help="candidates per user that --rec_dedup T starts from, K..128 (0, the default: min(128, 4 K))")
    p.add_argument("--rec_mmr", type=float, default=None,
                   help="LAMBDA in [0, 1] (only with --recommend K): ALSO lists re-ranked for diversity -- per user --rec_mmr_pool unseen "
                        "candidates are retrieved and K of them selected one by one by Maximal Marginal Relevance, LAMBDA x relevance - "
                        "(1 - LAMBDA) x cosine similarity to the nearest article already selected (helpers.diversify_lists); prints "
                        "hit@K / MRR / nDCG and the diversity of the plain and the re-ranked lists and saves "
                        "article_encoded_recommend{K}_mmr.npz.  The other output and files stay what they are")
    p.add_argument("--rec_mmr_pool", type=int, default=0,
                   help="candidates per user that --rec_mmr LAMBDA starts from, K..128 (0, the default: min(128, 4 K))")
    p.add_argument("--rec_max_per_label", type=int, default=0,
                   help="N > 0 (only with --rec_mmr LAMBDA): at most N articles of one label (the one --label names) per re-ranked list")
    p.add_argument("--rank_metrics", default=False, **b,
                   help="with --recommend K: also the rank of every held-out click among ALL unseen articles (no users x articles matrix), "
                        "saved to article_encoded_ranks.npz, and AUC, full MRR, mean / median rank and hit@{1, 10, 100} per model")
    p.add_argument("--session_decay", type=float, default=0.9,
                   help="decay of --recommend's user states: per click, or per unit of time when the sessions carry timestamps")
    p.add_argument("--fit_user_model", default=False, **b,
                   help="with --sessions S --recommend K: learn the user model's scaling vector alpha and its decay beta (start: "
                        "--session_decay) from the same histories by a pairwise ranking loss (helpers.fit_user_model), print the metrics "
                        "once more for the fitted model, and save alpha, beta and the loss history to user_model.npz")
    p.add_argument("--max_age", type=float, default=0.,
                   help="HOURS > 0 (only with --sessions synthetic --recommend K): the sessions get a timeline (articles in publication "
                        "order, clicks after publication), and every user is recommended, ranked and compared with the baseline only among "
                        "the articles published by the time of the held-out click and at most HOURS before it (`inf`: any age); the files "
                        "are article_encoded_recommend{K}_window.npz / article_encoded_ranks_window.npz.  0: off")
    p.add_argument("--user_model", default="decay", choices=["decay", "gru", "lstm", "rnn"],
                   help="the user model of --sessions S --recommend K.  decay (default): the decayed user states.  gru: ALSO the recurrent "
                        "user model -- GRU states (helpers.gru_user_states) from the weights in --gru_weights, through the same "
                        "recommend, --rank_metrics and --max_age paths; its files carry `_gru` in their names and its metrics are "
                        "printed beside the decay model's.  lstm / rnn: the same with the LSTM / plain-RNN states "
                        "(helpers.lstm_user_states / helpers.rnn_user_states) from the weights in --user_weights or trained by --fit_cell; files `_lstm` / `_rnn`")
    p.add_argument("--user_weights", default="",
                   help="with --user_model lstm / rnn: an .npz with weight_ih, weight_hh, bias_ih, bias_hh in the layout of torch.nn.LSTM / "
                        "torch.nn.RNN (helpers.LSTMUserModel / helpers.RNNUserModel; tools/gru_fit_torch.py --cell lstm / rnn writes one); "
                        "input and hidden size must equal the embedding size")
    p.add_argument("--gru_weights", default="",
                   help="an .npz with weight_ih, weight_hh, bias_ih, bias_hh in the layout of torch.nn.GRU (helpers.GRUUserModel; "
                        "tools/gru_fit_torch.py writes one); the hidden size must equal the embedding size")
    p.add_argument("--fit_gru", action="store_true",
                   help="with --user_model gru: train the GRU weights on the device (helpers.fit_gru_user_model) on the histories the "
                        "states are built from -- the held-out click is not among them -- print the loss per pair of every epoch and "
                        "save them as gru_user_model.npz; with --gru_weights the fit continues from those weights")
    p.add_argument("--gru_epochs", type=int, default=5, help="epochs of --fit_gru")
    p.add_argument("--fit_cell", action="store_true",
                   help="with --user_model lstm / rnn: train the cell's weights on the device (helpers.fit_lstm_user_model / "
                        "helpers.fit_rnn_user_model) on the histories the states are built from -- the held-out click is not among them -- and "
                        "save them as lstm_user_model.npz / rnn_user_model.npz; with --user_weights the fit continues from those weights")
    p.add_argument("--cell_epochs", type=int, default=5, help="epochs of --fit_cell")
    p.add_argument("--cell_validation", type=float, default=0.,
                   help="FRACTION in (0, 1) with --fit_cell: as --gru_validation, for the LSTM / plain-RNN fit")
    p.add_argument("--every_click", default=False, **b,
                   help="with --recommend K: beside the last-click evaluation (whose output and files stay what they are), rank EVERY click "
                        "of every session given the clicks before it (helpers.evaluate_every_click: one stamped seen-list per user, shared "
                        "by the user's rows) -- the decay model, the most-clicked-unseen baseline and, when selected, the fitted and GRU "
                        "models -- print the metrics and the table by clicks seen, and save rank / score / n_candidates / targets / "
                        "positions to article_encoded_every_click[_gru|_fitted][_window].npz; honours --max_age")
    p.add_argument("--gru_validation", type=float, default=0.,
                   help="FRACTION in (0, 1) with --fit_gru: hold out that share of the users (drawn by the fit's seed), train on the rest and "
                        "print the every-click MRR of the held-out users after every epoch (helpers.fit_gru_user_model(validation=...))")
    p.add_argument("--cluster", type=int, default=0,
                   help="K > 0: after encoding, spherical k-means of the train embeddings into K clusters on the device (helpers.kmeans): "
                        "iterations, mean score, cluster sizes and, with labels, purity / NMI / ARI against them; labels, centroids, counts "
                        "and history go to article_encoded_clusters.npz; with --validation the validation embeddings are assigned to the "
                        "same centroids")
    p.add_argument("--cluster_iters", type=int, default=50, help="centroid updates of --cluster K at the most")
    p.add_argument("--cluster_seed", type=int, default=0, help="seed of --cluster K's random start")
    p.add_argument("--cluster_n_init", type=int, default=1, help="restarts of --cluster K (seeds S, S + 1, ...); the best mean score is kept")
    p.add_argument("--ann_clusters", type=int, default=0,
                   help="C > 0 (only with --recommend K): ALSO the lists of a cluster index (helpers.ClusterIndex: k-means into C clusters, "
                        "every user scored against the articles of the --ann_probe nearest clusters only): recall@K against the exact "
                        "lists, hit / MRR / nDCG and the share of the corpus scored per user; saves article_encoded_recommend{K}_ann.npz")
    p.add_argument("--ann_probe", type=int, default=8, help="clusters probed per user by --ann_clusters C, 1..128")
    p.add_argument("--covisit", action="store_true",
                   help="with --sessions S --recommend K: ALSO the co-visitation baseline, readers of this article also read ... -- a "
                        "neighbour table built on the device from the co-clicks of the same histories (helpers.covisit_neighbors: no "
                        "embeddings, no articles x articles matrix), recommended from (CovisitIndex.recommend); prints hit@K / MRR / nDCG "
                        "as `co-visited articles` and the overlap of the co-click neighbours with the embedding neighbours "
                        "(helpers.list_overlap against helpers.most_similar), and saves article_encoded_recommend{K}_covisit.npz; honours "
                        "--max_age.  The other output and files stay what they are")
    p.add_argument("--covisit_window", type=int, default=3, help="W >= 1: two clicks of a user at most W positions apart co-occur (--covisit)")
    p.add_argument("--covisit_neighbors", type=int, default=50, help="N in 1..128: neighbours kept per article by --covisit")
    p.add_argument("--covisit_last", type=int, default=10, help="M in 1..32: the most recent clicks --covisit recommends from")
    p.add_argument("--als", action="store_true",
                   help="with --sessions S --recommend K: ALSO implicit-feedback matrix factorisation by alternating least squares, the "
                        "ID-based collaborative filter, trained on the device on the same histories (helpers.fit_als); prints hit@K / MRR / "
                        "nDCG as `ALS factors` (and its line of --rank_metrics), saves article_encoded_recommend{K}_als.npz and "
                        "als_model.npz; honours --max_age.  The other output and files stay what they are")
    p.add_argument("--words", action="store_true",
                   help="with --sessions S --recommend K: ALSO the paper's word-based model -- an article is the set of its words (the "
                        "train matrix the autoencoder was fed, binary or tf-idf per --input_format), a user the set of the words of the "
                        "articles clicked, the relevance the weighted count of shared words (helpers.word_recommend: bitmap profiles, "
                        "sparse on both sides); prints hit@K / MRR / nDCG as `word-based model` (and its line of --rank_metrics), saves "
                        "article_encoded_recommend{K}_words.npz (and article_encoded_ranks_words.npz); honours --max_age.  The other "
                        "output and files stay what they are")
    p.add_argument("--words_idf", action="store_true", help="--words: weight every word by its smooth idf (helpers.idf_weights)")
    p.add_argument("--words_last", type=int, default=0, help="M > 0: --words builds a profile from the user's last M clicks only (0: all)")
    p.add_argument("--als_factors", type=int, default=64, help="F in 1..128: the number of factors of --als")
    p.add_argument("--als_iterations", type=int, default=15, help="iterations of --als (a user and an article half-sweep each)")
    p.add_argument("--als_alpha", type=float, default=40.0, help="the confidence of a click of --als: c = 1 + alpha * clicks")
    p.add_argument("--als_reg", type=float, default=0.01, help="the regularisation lambda of --als")
    return p


def validate(a):
    """The reference's asserts (:94-109)."""
    assert 0. <= a.min_df <= 1.
    assert 0. <= a.max_df <= 1.
    assert a.max_features >= 1
    assert 0. <= a.corr_frac <= 1.
    assert a.verbose_step > 0
    if a.input_format == 'tfidf':
        assert a.loss_func in ['mean_squared', 'cosine_proximity']
    if a.main_dir == '':
        a.main_dir = a.model_name
    assert a.model_name != '', "--model_name is required"
    assert a.recommend == 0 or a.sessions != '', "--recommend needs --sessions"
    assert 0. <= a.session_decay <= 1.
    assert not a.rank_metrics or a.recommend > 0, "--rank_metrics needs --recommend K"
    assert a.rec_dedup is None or a.recommend > 0, "--rec_dedup needs --recommend K"
    assert a.rec_dedup_pool == 0 or a.rec_dedup is not None, "--rec_dedup_pool needs --rec_dedup T"
    assert a.rec_dedup_pool == 0 or a.recommend <= a.rec_dedup_pool <= 128, "--rec_dedup_pool is a number in K..128"
    assert a.rec_mmr is None or (a.recommend > 0 and 0. <= a.rec_mmr <= 1.), "--rec_mmr LAMBDA needs --recommend K and LAMBDA in [0, 1]"
    assert a.rec_mmr_pool == 0 or a.rec_mmr is not None, "--rec_mmr_pool needs --rec_mmr LAMBDA"
    assert a.rec_mmr_pool == 0 or a.recommend <= a.rec_mmr_pool <= 128, "--rec_mmr_pool is a number in K..128"
    assert a.rec_max_per_label >= 0 and (a.rec_max_per_label == 0 or a.rec_mmr is not None), "--rec_max_per_label N needs --rec_mmr LAMBDA"
    assert not a.fit_user_model or (a.sessions != '' and a.recommend > 0), "--fit_user_model needs --sessions S --recommend K"
    assert a.user_model != 'gru' or (a.sessions != '' and a.recommend > 0 and (a.gru_weights != '' or a.fit_gru)), \
        "--user_model gru needs --sessions S --recommend K and --gru_weights PATH or --fit_gru"
    assert a.user_model not in ('lstm', 'rnn') or (a.sessions != '' and a.recommend > 0 and (a.user_weights != '' or a.fit_cell)), \
        "--user_model lstm / rnn needs --sessions S --recommend K and --user_weights PATH or --fit_cell"
    assert not a.fit_cell or a.user_model in ('lstm', 'rnn'), "--fit_cell needs --user_model lstm or rnn (the GRU has --fit_gru, the decay model --fit_user_model)"
    assert a.cell_epochs >= 0
    assert 0. <= a.cell_validation < 1., "--cell_validation is a fraction in [0, 1)"
    assert a.cell_validation == 0. or a.fit_cell, "--cell_validation needs --fit_cell"
    assert not a.fit_gru or a.user_model == 'gru', "--fit_gru needs --user_model gru"
    assert a.gru_epochs >= 0
    assert not a.every_click or a.recommend > 0, "--every_click needs --recommend K"
    assert 0. <= a.gru_validation < 1., "--gru_validation is a fraction in [0, 1)"
    assert a.gru_validation == 0. or a.fit_gru, "--gru_validation needs --fit_gru"
    assert a.max_age >= 0., "--max_age is a number of hours"
    assert a.cluster >= 0 and a.cluster_iters >= 0 and a.cluster_n_init >= 1, "--cluster K, --cluster_iters I >= 0, --cluster_n_init R >= 1"
    assert a.ann_clusters == 0 or (a.ann_clusters > 0 and a.recommend > 0 and a.max_age == 0.), \
        "--ann_clusters C needs --recommend K (and does not go with --max_age: an index takes no windows)"
    assert 1 <= a.ann_probe <= 128, "--ann_probe is a number in 1..128"
    assert not a.covisit or (a.sessions != '' and a.recommend > 0), "--covisit needs --sessions S --recommend K"
    assert not a.words or (a.sessions != '' and a.recommend > 0), "--words needs --sessions S --recommend K"
    assert a.words or not (a.words_idf or a.words_last), "--words_idf and --words_last M belong to --words"
    assert a.words_last >= 0, "--words_last M >= 0"
    assert a.covisit_window >= 1 and 1 <= a.covisit_neighbors <= 128 and 1 <= a.covisit_last <= 32, \
        "--covisit_window W >= 1, --covisit_neighbors N in 1..128, --covisit_last M in 1..32"
    assert a.max_age == 0. or (a.sessions == 'synthetic' and a.recommend > 0), "--max_age needs --sessions synthetic --recommend K"
    assert not a.als or (a.sessions != '' and a.recommend > 0), "--als needs --sessions S --recommend K"
    assert 1 <= a.als_factors <= 128 and a.als_iterations >= 0 and a.als_alpha >= 0. and a.als_reg >= 0., \
        "--als_factors F in 1..128, --als_iterations N >= 0, --als_alpha A >= 0, --als_reg L >= 0"
    return a


def load_data(a):
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_csr, synthetic_labels
    n = a.train_row + (a.validate_row if a.validation else 0)
    if a.data:
        X = sparse.load_npz(a.data).tocsr() if a.data.endswith(".npz") else np.load(a.data)
        y = np.load(a.labels, allow_pickle=True) if a.labels else None
        X = X[:n]; y = None if y is None else y[:n]
    else:
        seed = a.seed if a.seed >= 0 else 1234
        X = synthetic_csr(n, a.max_features, nnz_per_row=200, seed=seed, tfidf=(a.input_format == "tfidf"))
        y = synthetic_labels(n, kind="category" if a.label == "category_publish_name" else "story", seed=seed)
    if a.input_format == "binary" and sparse.issparse(X):
        X.data[:] = 1                                                   # reference :235-236
    return X, y


def evaluate_similarity(a, trX, vlX, trY, vlY, emb, emb_v, plot_dir=None):
    """Reference :307-317 + :322-345 -- pairwise cosine similarity of the input vectors and of the embeddings (train,
    validation) and, per label, the related-vs-unrelated comparison the reference draws as ROC curve + box plot
    (helpers.visualize_pairwise_similarity).  Both run on the MI355X (dae_pairwise_similarity, dae_pair_stats); the figure's
    numbers are printed and, with ``plot_dir``, written as JSON under the reference's figure names."""
    from dae_rnn_news_recommendation_amd import helpers
    print('calculate similarity')
    metric_in = 'linear kernel' if a.input_format == 'tfidf' else 'cosine'   # TF-IDF rows are l2-normalised already (:311)
    stem_in = 'tfidf' if a.input_format == 'tfidf' else 'binary_count'
    jobs = [('input vectors (train)', trX, metric_in, trY, 'similarity_boxplot_' + stem_in),
            ('embedding (train)', emb, 'cosine', trY, 'similarity_boxplot_encoded')]
    if vlX is not None:
        jobs += [('input vectors (validate)', vlX, metric_in, vlY, 'similarity_boxplot_' + stem_in + '_validate'),
                 ('embedding (validate)', emb_v, 'cosine', vlY, 'similarity_boxplot_encoded_validate')]
    rows = []
    for name, M, metric, y, fig in jobs:
        S = helpers.pairwise_similarity(M, metric=metric, return_tensor=True)
        line = '  %-26s %5d x %-5d' % (name, S.shape[0], S.shape[1])
        if y is not None:
            ids = np.unique(np.asarray(y), return_inverse=True)[1]
            st = helpers.visualize_pairwise_similarity(ids, S, plot='boxplot', title=name,
                                                       save_path=None if plot_dir is None else plot_dir + fig + '.png')
            line += '  AUROC %.4f  median sim related %.4f  unrelated %.4f  (%d / %d pairs)' % (
                st['auroc'], st['related']['median'] if st['n_related'] else float('nan'),
                st['unrelated']['median'] if st['n_unrelated'] else float('nan'), st['n_related'], st['n_unrelated'])
            rows.append((name, st))
        print(line)
        del S
    print('calculate similarity done')
    return rows


def sweep_chunk_rows_arg(a):
    """--sweep_chunk_rows as the ``chunk_rows`` of helpers.most_similar / label_similarity_stats: 0 -> None, -1 -> 'auto'."""
    n = int(getattr(a, 'sweep_chunk_rows', 0) or 0)
    assert n >= -1, "--sweep_chunk_rows must be 0, -1 (auto) or a positive row count"
    return None if n == 0 else 'auto' if n < 0 else n


def evaluate_label_stats(a, trX, vlX, trY, vlY, emb, emb_v, plot_dir=None):
    """--label_stats: the four jobs of evaluate_similarity through helpers.label_similarity_stats (dae_pair_hist: per-class score
    histograms in the GEMM's epilogue, no N x N matrix).  Prints the same per-job line with the AUROC's bracket appended and, with
    ``plot_dir``, writes similarity_stats_<name>.json."""
    from dae_rnn_news_recommendation_amd import helpers
    assert trY is not None, "--label_stats needs labels"
    print('calculate label statistics')
    metric_in = 'linear kernel' if a.input_format == 'tfidf' else 'cosine'
    stem_in = 'tfidf' if a.input_format == 'tfidf' else 'binary_count'
    jobs = [('input vectors (train)', trX, metric_in, trY, stem_in), ('embedding (train)', emb, 'cosine', trY, 'encoded')]
    if vlX is not None and vlY is not None:
        jobs += [('input vectors (validate)', vlX, metric_in, vlY, stem_in + '_validate'),
                 ('embedding (validate)', emb_v, 'cosine', vlY, 'encoded_validate')]
    rows = []
    for name, M, metric, y, stem in jobs:
        ids = np.unique(np.asarray(y), return_inverse=True)[1]
        st = helpers.label_similarity_stats(M, ids, metric=metric, title=name, chunk_rows=sweep_chunk_rows_arg(a),
                                            save_path=None if plot_dir is None else plot_dir + 'similarity_stats_' + stem + '.png')
        print('  %-26s %5d x %-5d  AUROC %.4f  median sim related %.4f  unrelated %.4f  (%d / %d pairs)  AUROC in [%.6f, %.6f]' % (
            name, M.shape[0], M.shape[0], st['auroc'], st['related']['median'], st['unrelated']['median'], st['n_related'],
            st['n_unrelated'], st['auroc_low'], st['auroc_high']))
        rows.append((name, st))
    print('calculate label statistics done')
    return rows


def evaluate_top_k(a, trX, vlX, trY, vlY, emb, emb_v, data_dir):
    """--top_k K: the K nearest train articles of every train article (itself excluded) and of every validation article, by
    the cosine of the embeddings (helpers.most_similar, no N x N matrix), saved as ``indices`` / ``scores`` in
    article_encoded[_validate]_top{K}.npz; with labels, precision@K of the input vectors (the metric of evaluate_similarity)
    against that of the embedding."""
    from dae_rnn_news_recommendation_amd import helpers
    K = a.top_k
    print('calculate top %d' % K)
    metric_in = 'linear kernel' if a.input_format == 'tfidf' else 'cosine'
    sets = [('train', trX, emb, trY, None, None, None, 'article_encoded_top%d.npz' % K)]
    if emb_v is not None:
        sets.append(('validate', vlX, emb_v, vlY, trX, emb, trY, 'article_encoded_validate_top%d.npz' % K))
    out = {}
    for name, X, E, y, Xc, Ec, yc, fname in sets:
        idx, score = helpers.most_similar(E, k=K, candidates=Ec, chunk_rows=sweep_chunk_rows_arg(a))
        np.savez(data_dir + fname, indices=idx, scores=score)
        out[name] = idx
        print('  %-9s %5d queries -> %s' % (name, idx.shape[0], fname))
        if y is not None:
            idx_in, _ = helpers.most_similar(X, k=K, metric=metric_in, candidates=Xc, chunk_rows=sweep_chunk_rows_arg(a))
            p_in, n = helpers.label_precision_at_k(idx_in, y, yc)
            p_emb, _ = helpers.label_precision_at_k(idx, y, yc)
            print('  precision@%d %-9s input vectors %.4f  embedding %.4f  (%d queries)' % (K, name, p_in, p_emb, n))
    print('calculate top %d done' % K)
    return out


def evaluate_duplicates(a, trY, vlY, emb, emb_v, data_dir):
    """--dup_threshold T: the pairs of train articles whose embeddings have cosine >= T (helpers.similar_pairs, no N x N matrix),
    saved with their connected components (``group``: first article of the story, ``keep``: that article) in
    article_encoded_dups.npz; validation articles against the train corpus in article_encoded_validate_dups.npz (pairs only).
    With labels, the share of pairs whose two labels are equal."""
    from dae_rnn_news_recommendation_amd import helpers
    T = a.dup_threshold
    print('calculate duplicates at cosine >= %g' % T)
    out = {}
    rows, cols, scores = helpers.similar_pairs(emb, T)
    group, keep = helpers.duplicate_groups(rows, cols, emb.shape[0])
    np.savez(data_dir + 'article_encoded_dups.npz', rows=rows, cols=cols, scores=scores, group=group, keep=keep, threshold=np.float32(T))
    out['train'] = (rows, cols, scores, group, keep)
    line = '  train     %d pairs, %d groups of more than one article, %d articles dropped' % (
        rows.shape[0], int((np.bincount(group, minlength=1) > 1).sum()), int((~keep).sum()))
    if trY is not None:
        line += ', pair precision %.4f (%d pairs)' % helpers.duplicate_pair_precision(rows, cols, trY)
    print(line)
    if emb_v is not None:
        rows, cols, scores = helpers.similar_pairs(emb_v, T, candidates=emb)
        np.savez(data_dir + 'article_encoded_validate_dups.npz', rows=rows, cols=cols, scores=scores, threshold=np.float32(T))
        out['validate'] = (rows, cols, scores)
        line = '  validate  %d pairs with train articles, %d of %d validation articles have one' % (
            rows.shape[0], np.unique(rows).shape[0], emb_v.shape[0])
        if vlY is not None and trY is not None:
            line += ', pair precision %.4f (%d pairs)' % helpers.duplicate_pair_precision(rows, cols, vlY, trY)
        print(line)
    print('calculate duplicates done')
    return out


def evaluate_recommend(a, trY, emb, data_dir, trX=None):
    """--sessions S --recommend K: next-click evaluation of the decaying user model.  Every user's last click is held out; the
    user state is the decay-weighted mean of the train embeddings of the clicks before it (helpers.user_states); the K unseen
    articles with the largest inner product are recommended (helpers.recommend: no users x articles matrix) and saved as
    ``indices`` / ``scores`` / ``targets`` in article_encoded_recommend{K}.npz.  hit@K, MRR@K and nDCG@K are printed beside
    those of the most-clicked-unseen baseline (host code).  Users with fewer than two clicks have no target (-1) and are not
    counted.

    With --max_age HOURS the sessions carry a timeline (synthetic_timed_sessions), the user states decay per hour, and the time
    of the held-out click gives every user a candidate window (helpers.candidate_windows): the model and the baseline recommend
    only among the articles published by then and at most HOURS earlier.  The file is article_encoded_recommend{K}_window.npz
    and also holds ``window_lo`` / ``window_hi`` / ``max_age`` / ``mean_window``."""
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_sessions
    K, n = a.recommend, emb.shape[0]
    print('calculate recommend %d' % K)
    t = None
    if a.max_age > 0:
        return evaluate_recommend_window(a, trY, emb, data_dir, trX)
    if a.sessions == 'synthetic':
        assert trY is not None, "--sessions synthetic needs labels"
        seed = a.seed if a.seed >= 0 else 1234
        indptr, items = synthetic_sessions(max(n // 2, 1), np.unique(np.asarray(trY), return_inverse=True)[1], mean_len=12, seed=seed)
    else:
        with np.load(a.sessions) as f:
            indptr, items = np.asarray(f['indptr'], dtype=np.int64), np.asarray(f['items'])
            t = np.asarray(f['timestamps'], dtype=np.float64) if 'timestamps' in f.files else None
    lens = np.diff(indptr)
    users = lens.shape[0]
    has = lens >= 2
    targets = np.where(has, items[np.maximum(indptr[1:] - 1, 0)] if items.size else -1, -1).astype(np.int64)
    keep = np.ones(items.shape[0], dtype=bool)
    keep[indptr[1:][lens >= 1] - 1] = False                               # the history is everything before the last click
    h_ptr = np.zeros(users + 1, dtype=np.int64)
    h_ptr[1:] = np.cumsum(np.maximum(lens - 1, 0))
    hist = (h_ptr, items[keep])
    states = helpers.user_states(hist, emb, a.session_decay, timestamps=None if t is None else t[keep], return_tensor=True)
    idx, score = helpers.recommend(states, emb, k=K, seen=hist)
    np.savez(data_dir + 'article_encoded_recommend%d.npz' % K, indices=idx, scores=score, targets=targets)
    m = helpers.next_click_metrics(idx, targets)
    b = helpers.next_click_metrics(helpers.popularity_recommend(hist, n, K), targets)
    print('  %d users, %d clicks, %d with a held-out click -> article_encoded_recommend%d.npz' % (users, items.shape[0], m['n'], K))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'decayed user state', m['hit'], m['mrr'], m['ndcg']))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'most clicked unseen', b['hit'], b['mrr'], b['ndcg']))
    print('calculate recommend %d done' % K)
    if a.rec_dedup is not None:
        evaluate_recommend_dedup(a, states, emb, hist, targets, data_dir)
    if a.rec_mmr is not None:
        evaluate_recommend_mmr(a, trY, states, emb, hist, targets, data_dir)
    if a.ann_clusters > 0:
        evaluate_recommend_ann(a, states, emb, hist, idx, targets, data_dir)
    if a.covisit:
        evaluate_recommend_covisit(a, emb, hist, targets, data_dir)
    if a.als:
        evaluate_recommend_als(a, hist, targets, n, data_dir)
    if a.words:
        evaluate_recommend_words(a, trX, hist, targets, data_dir)
    models = {}
    if a.rank_metrics:
        evaluate_rank_metrics(states, emb, hist, targets, n, data_dir)
    if a.fit_user_model:
        models['fitted'] = evaluate_fitted_user_model(a, emb, hist, targets, n, data_dir, timestamps=None if t is None else t[keep])
    if a.user_model != 'decay':
        evaluate_recurrent_user_model(a, emb, hist, targets, n, data_dir, models=models)
    if a.every_click:
        evaluate_every_click(a, emb, (indptr, items), t, None, models, data_dir)
    return idx, score, targets


def evaluate_recommend_ann(a, states, emb, hist, exact, targets, data_dir):
    """--ann_clusters C [--ann_probe P]: the lists of evaluate_recommend once more through a cluster index (helpers.ClusterIndex:
    k-means of the train embeddings into C clusters; every user state is scored against the unseen articles of its P nearest
    clusters only -- for the inner product the choice of clusters is a heuristic).  Prints recall@K against the exact lists, hit@K /
    MRR@K / nDCG@K and the share of the corpus scored per user; saves ``indices`` / ``scores`` / ``targets`` / ``order`` / ``offsets``
    / ``centroids`` to article_encoded_recommend{K}_ann.npz."""
    from dae_rnn_news_recommendation_amd import helpers
    K, C, P = a.recommend, min(a.ann_clusters, emb.shape[0]), a.ann_probe
    print('calculate recommend %d through %d clusters, %d probed' % (K, C, P))
    index = helpers.ClusterIndex.build(emb, C, '', 'linear kernel', max_iter=a.cluster_iters, seed=a.cluster_seed)
    idx, score = index.search(states, K, n_probe=P, exclude=hist)
    exact = np.asarray(exact)
    found = ((idx[:, :, None] == exact[:, None, :]) & (idx[:, :, None] >= 0)).any(axis=2).sum()
    recall = found / max(int((exact >= 0).sum()), 1)
    name = 'article_encoded_recommend%d_ann.npz' % K
    np.savez(data_dir + name, indices=idx, scores=score, targets=targets, order=index.order, offsets=index.offsets, centroids=index.centroids,
             n_probe=np.int64(P))
    m = helpers.next_click_metrics(idx, targets)
    print('  recall@%d against the exact lists %.4f, %.4f of the corpus scored per user -> %s' % (K, recall, index.probed_fraction(states, P), name))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'cluster index', m['hit'], m['mrr'], m['ndcg']))
    print('calculate recommend through clusters done')
    return idx, score


def evaluate_recommend_covisit(a, emb, hist, targets, data_dir, window=None):
    """--covisit: the co-visitation baseline beside the embedding models.  The neighbour table is built on the device from the
    co-clicks of the histories the other models see -- the held-out click is not among them -- (helpers.covisit_neighbors:
    --covisit_window, both directions, cosine, --covisit_neighbors per article) and every user is recommended the K unseen articles
    the neighbours of the last --covisit_last clicks point at (CovisitIndex.recommend; with ``window`` inside the candidate windows
    of --max_age).  Prints hit@K / MRR@K / nDCG@K as `co-visited articles` and the share of an article's co-click neighbours that
    are also among its nearest embedding neighbours (helpers.list_overlap against helpers.most_similar).  Saves ``indices`` /
    ``scores`` / ``targets`` / ``hist_indptr`` / ``hist_items`` / ``neighbors`` / ``sims`` / ``counts`` to
    article_encoded_recommend{K}[_window]_covisit.npz."""
    from dae_rnn_news_recommendation_amd import helpers
    K, n, N = a.recommend, emb.shape[0], a.covisit_neighbors
    name = 'article_encoded_recommend%d%s_covisit.npz' % (K, '' if window is None else '_window')
    print('calculate recommend %d covisit' % K)
    index = helpers.covisit_neighbors(hist, n, window=a.covisit_window, n_neighbors=N)
    idx, score = index.recommend(hist, K, last=a.covisit_last, window=window)
    np.savez(data_dir + name, indices=idx, scores=score, targets=targets, hist_indptr=hist[0], hist_items=hist[1],
             neighbors=index.neighbors, sims=index.sims, counts=index.counts)
    m = helpers.next_click_metrics(idx, targets)
    print('  window %d, %d neighbours, last %d clicks: %d records, %d distinct pairs, %.1f neighbours per article -> %s' % (
        a.covisit_window, N, a.covisit_last, index.n_records, index.n_pairs, float(index.degree.mean()), name))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'co-visited articles', m['hit'], m['mrr'], m['ndcg']))
    near = helpers.most_similar(emb, k=min(N, max(n - 1, 1)))[0]
    print('  co-click neighbours among the %d nearest embedding neighbours: %.4f' % (near.shape[1], helpers.list_overlap(index.neighbors, near)[1]))
    print('calculate recommend %d covisit done' % K)
    return idx, score


def evaluate_recommend_als(a, hist, targets, n, data_dir, window=None):
    """--als: implicit-feedback matrix factorisation beside the embedding models.  The factors are fitted on the device to the
    histories the other models see -- the held-out click is not among them -- (helpers.fit_als: --als_factors, --als_iterations,
    --als_alpha, --als_reg) and every user is recommended the K unseen articles with the largest inner product of the user's and
    the article's factors (ALSModel.recommend; with ``window`` inside the candidate windows of --max_age).  Prints hit@K / MRR@K /
    nDCG@K as `ALS factors`, and with --rank_metrics the line of evaluate_rank_metrics for the same model.  Saves ``indices`` /
    ``scores`` / ``targets`` / ``hist_indptr`` / ``hist_items`` (and ``rank`` / ``n_candidates`` with --rank_metrics) to
    article_encoded_recommend{K}[_window]_als.npz and the model to als_model.npz."""
    from dae_rnn_news_recommendation_amd import helpers
    K = a.recommend
    name = 'article_encoded_recommend%d%s_als.npz' % (K, '' if window is None else '_window')
    print('calculate recommend %d als' % K)
    model = helpers.fit_als(hist, n, factors=a.als_factors, regularization=a.als_reg, alpha=a.als_alpha, iterations=a.als_iterations,
                            compute_loss=True)
    idx, score = model.recommend(hist, K, window=window)
    extra = {}
    m = helpers.next_click_metrics(idx, targets)
    curve = model.loss_curve
    print('  %d factors, %d iterations, alpha %g, lambda %g: loss %s -> %s' % (
        model.factors, model.iterations, model.alpha, model.regularization,
        '%.6g to %.6g' % (curve[0], curve[-1]) if curve else 'not computed', name))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'ALS factors', m['hit'], m['mrr'], m['ndcg']))
    if a.rank_metrics:
        rank, _, n_cand = helpers.recommend_ranks(model.user_states(hist), model.item_factors, targets, seen=hist, window=window)
        r = helpers.rank_metrics(rank, n_cand, targets, ks=(1, 10, 100))
        print('  ranks %-20s AUC %.4f  MRR %.4f  mean rank %.1f  median rank %.1f  hit@1 %.4f  hit@10 %.4f  hit@100 %.4f'
              % ('ALS factors', r['auc'], r['mrr'], r['mean_rank'], r['median_rank'], r['hit@1'], r['hit@10'], r['hit@100']))
        extra = dict(rank=rank, n_candidates=n_cand)
    np.savez(data_dir + name, indices=idx, scores=score, targets=targets, hist_indptr=hist[0], hist_items=hist[1], **extra)
    model.save(data_dir + 'als_model.npz')
    print('calculate recommend %d als done' % K)
    return idx, score


def evaluate_recommend_words(a, trX, hist, targets, data_dir, window=None):
    """--words: the paper's word-based model beside the embedding models.  An article is the set of the words of its row of the
    train matrix ``trX`` (what the autoencoder was fed: binary or tf-idf per --input_format), a user the set of the words of the
    articles of the history the other models see -- the held-out click is not among them; --words_last M: of its last M clicks --
    and every user is recommended the K unseen articles with the largest sum of the article's entries over the shared words
    (helpers.word_recommend; --words_idf: every entry times the word's smooth idf, helpers.idf_weights; with ``window`` inside the
    candidate windows of --max_age).  Prints hit@K / MRR@K / nDCG@K as `word-based model`, and with --rank_metrics the line of
    evaluate_rank_metrics for the same model (helpers.word_ranks; a re-click of an article of the history counts as a miss, as it
    does for the other models).  Saves ``indices`` / ``scores`` / ``targets`` / ``hist_indptr`` / ``hist_items`` /
    ``profile_sizes`` to article_encoded_recommend{K}[_window]_words.npz and, with --rank_metrics, ``rank`` / ``score`` /
    ``n_candidates`` / ``targets`` to article_encoded_ranks[_window]_words.npz."""
    import scipy.sparse as sp
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.helpers.sweeps import competitors
    K = a.recommend
    tag = '' if window is None else '_window'
    name = 'article_encoded_recommend%d%s_words.npz' % (K, tag)
    print('calculate recommend %d words' % K)
    articles = sp.csr_matrix(trX, dtype=np.float32)
    articles.sum_duplicates()
    articles.sort_indices()
    n, V = articles.shape
    weights = helpers.idf_weights(articles) if a.words_idf else None
    last = a.words_last if a.words_last > 0 else None
    profiles = helpers.word_profiles(hist, articles, max_events=last)
    idx, score = helpers.word_recommend(profiles, articles, K, seen=hist, term_weights=weights, window=window)
    np.savez(data_dir + name, indices=idx, scores=score, targets=targets, hist_indptr=hist[0], hist_items=hist[1], profile_sizes=profiles.sizes)
    m = helpers.next_click_metrics(idx, targets)
    print('  %d words, %.1f per article, %.1f per profile%s%s -> %s' % (
        V, articles.nnz / max(n, 1), float(profiles.sizes.mean()) if profiles.sizes.size else 0.0, ', idf weights' if a.words_idf else '',
        ', last %d clicks' % last if last else '', name))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'word-based model', m['hit'], m['mrr'], m['ndcg']))
    if a.rank_metrics:
        rank, t_score, n_cand = helpers.word_ranks(profiles, articles, targets, seen=hist, term_weights=weights, window=window)
        rank = np.where(competitors(targets, len(targets), n, False, *helpers.normalize_exclusions(hist, len(targets), n), window)[1],
                        0, rank)                                       # a target the user can never be shown: a miss
        r = helpers.rank_metrics(rank, n_cand, targets, ks=(1, 10, 100))
        print('  ranks %-20s AUC %.4f  MRR %.4f  mean rank %.1f  median rank %.1f  hit@1 %.4f  hit@10 %.4f  hit@100 %.4f'
              % ('word-based model', r['auc'], r['mrr'], r['mean_rank'], r['median_rank'], r['hit@1'], r['hit@10'], r['hit@100']))
        np.savez(data_dir + 'article_encoded_ranks%s_words.npz' % tag, rank=rank, score=t_score, n_candidates=n_cand, targets=targets)
    print('calculate recommend %d words done' % K)
    return idx, score


def evaluate_clusters(a, trY, vlY, emb, emb_v, data_dir):
    """--cluster K: spherical k-means of the train embeddings (helpers.kmeans, on the device): iterations, mean score, the largest
    and the smallest cluster and the empty clusters relocated; with labels purity / NMI / ARI against them
    (helpers.cluster_label_scores).  ``labels`` / ``centroids`` / ``counts`` / ``scores`` / ``history`` go to
    article_encoded_clusters.npz.  The validation embeddings are assigned to the same centroids (helpers.kmeans_assign) and scored the
    same way; their ``labels`` / ``scores`` go to article_encoded_validate_clusters.npz."""
    from dae_rnn_news_recommendation_amd import helpers
    K = min(a.cluster, emb.shape[0])
    print('calculate clusters %d' % K)
    res = helpers.kmeans(emb, K, max_iter=a.cluster_iters, seed=a.cluster_seed, n_init=a.cluster_n_init)
    np.savez(data_dir + 'article_encoded_clusters.npz', labels=res.labels, centroids=res.centroids, counts=res.counts, scores=res.scores,
             history=np.asarray(res.history, dtype=np.float64))

    def against(labels, true):
        if true is None:
            return ''
        s = helpers.cluster_label_scores(labels, np.unique(np.asarray(true), return_inverse=True)[1])
        return '  purity %.4f  NMI %.4f  ARI %.4f (%d articles, %d labels)' % (s['purity'], s['nmi'], s['ari'], s['n'], s['n_labels'])
    print('  train     %d iterations, mean score %.6f, clusters of %d .. %d articles, %d empty clusters relocated%s -> '
          'article_encoded_clusters.npz' % (res.n_iter, res.mean_score, int(res.counts.min()), int(res.counts.max()), res.relocated,
                                            against(res.labels, trY)))
    if emb_v is not None:
        lab_v, score_v = helpers.kmeans_assign(emb_v, res.centroids)
        np.savez(data_dir + 'article_encoded_validate_clusters.npz', labels=lab_v, scores=score_v)
        sizes = np.bincount(lab_v, minlength=K)
        print('  validate  mean score %.6f, clusters of %d .. %d articles%s -> article_encoded_validate_clusters.npz'
              % (float(score_v.astype(np.float64).mean()), int(sizes.min()), int(sizes.max()), against(lab_v, vlY)))
    print('calculate clusters done')
    return res


def evaluate_recommend_dedup(a, states, emb, hist, targets, data_dir, window=None):
    """--rec_dedup T: the lists of evaluate_recommend once more with the pipeline's last stage, near-duplicates dropped
    (helpers.recommend(dedup_threshold=T): --rec_dedup_pool candidates per user, walked best first down to K; cosine similarity of
    the embeddings).  Prints hit@K / MRR@K / nDCG@K of those lists and the mean number of duplicate pairs per list before -- among
    the plain top-K -- and after: the de-duplicated lists handed to helpers.dedup_lists again, which must find none.  Saves
    ``indices`` / ``scores`` / ``targets`` / ``n_kept`` / ``dup_pairs_before`` to article_encoded_recommend{K}[_window]_dedup.npz."""
    from dae_rnn_news_recommendation_amd import helpers
    K, T = a.recommend, a.rec_dedup
    pool = a.rec_dedup_pool if a.rec_dedup_pool > 0 else min(128, 4 * K)
    name = 'article_encoded_recommend%d%s_dedup.npz' % (K, '' if window is None else '_window')
    print('calculate recommend %d dedup %g' % (K, T))
    cand, cand_score = helpers.recommend(states, emb, k=pool, seen=hist, window=window, return_tensor=True)
    idx, score, (n_kept, before) = helpers.dedup_lists(cand, emb, K, T, scores=cand_score, return_counts=True)
    _, _, (_, after) = helpers.dedup_lists(idx, emb, K, T, return_counts=True)
    np.savez(data_dir + name, indices=idx, scores=score, targets=targets, n_kept=n_kept, dup_pairs_before=before)
    m = helpers.next_click_metrics(idx, targets)
    print('  pool %d, cosine >= %g: %.2f kept per list -> %s' % (pool, T, float(n_kept.mean()) if n_kept.size else 0.0, name))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'dedup user state', m['hit'], m['mrr'], m['ndcg']))
    print('  duplicate pairs per list: before %.4f  after %.4f' % (float(before.mean()) if before.size else 0.0,
                                                                  float(after.mean()) if after.size else 0.0))
    assert int(after.sum()) == 0, "a de-duplicated list still holds a duplicate pair"
    print('calculate recommend %d dedup done' % K)
    return idx, score


def evaluate_recommend_mmr(a, trY, states, emb, hist, targets, data_dir, window=None):
    """--rec_mmr LAMBDA: the lists of evaluate_recommend once more, re-ranked for diversity (helpers.diversify_lists: Maximal
    Marginal Relevance with weight LAMBDA over --rec_mmr_pool candidates per user, their relevance rescaled per list to [0, 1],
    cosine similarity of the embeddings; with --rec_max_per_label N at most N articles of one --label per list).  Prints
    hit@K / MRR@K / nDCG@K of the plain and the diversified lists and helpers.list_diversity of both: the mean similarity of a
    list's entries to the nearest entry before them and, with labels, the labels per list and the largest share of one label.
    Saves ``indices`` / ``scores`` / ``targets`` / ``n_selected`` / ``n_beyond_topk`` / ``nearest`` to
    article_encoded_recommend{K}[_window]_mmr.npz."""
    from dae_rnn_news_recommendation_amd import helpers
    K, lam, cap = a.recommend, a.rec_mmr, a.rec_max_per_label
    pool = a.rec_mmr_pool if a.rec_mmr_pool > 0 else min(128, 4 * K)
    name = 'article_encoded_recommend%d%s_mmr.npz' % (K, '' if window is None else '_window')
    labels = None if trY is None else np.unique(np.asarray(trY), return_inverse=True)[1]
    assert cap == 0 or labels is not None, "--rec_max_per_label needs labels"
    print('calculate recommend %d mmr %g' % (K, lam))
    cand, cand_score = helpers.recommend(states, emb, k=pool, seen=hist, window=window, return_tensor=True)
    plain, _, p = helpers.diversify_lists(cand, cand_score, emb, K, 1.0, return_details=True)       # lambda = 1: the plain top-K
    idx, score, d = helpers.diversify_lists(cand, cand_score, emb, K, lam, labels=labels, max_per_label=cap if cap > 0 else None,
                                            scale_relevance='minmax', return_details=True)
    np.savez(data_dir + name, indices=idx, scores=score, targets=targets, n_selected=d['n_selected'], n_beyond_topk=d['n_beyond_topk'],
             nearest=d['nearest'])
    mean = lambda x: float(x.mean()) if x.size else 0.0
    before, after = helpers.list_diversity(plain, p['nearest'], labels), helpers.list_diversity(idx, d['nearest'], labels)
    m0, m = helpers.next_click_metrics(plain, targets), helpers.next_click_metrics(idx, targets)
    print('  pool %d, lambda %g%s: %.2f selected per list, %.2f of them from beyond the top %d -> %s' % (
        pool, lam, ', at most %d per label' % cap if cap > 0 else '', mean(d['n_selected']), mean(d['n_beyond_topk']), K, name))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'plain user state', m0['hit'], m0['mrr'], m0['ndcg']))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'mmr user state', m['hit'], m['mrr'], m['ndcg']))
    print('  nearest similarity in a list: before %.4f  after %.4f' % (before['mean_nearest'], after['mean_nearest']))
    if labels is not None:
        print('  labels per list: before %.2f  after %.2f; largest label share: before %.4f  after %.4f' % (
            before['mean_n_labels'], after['mean_n_labels'], before['mean_max_label_share'], after['mean_max_label_share']))
    print('calculate recommend %d mmr done' % K)
    return idx, score


def evaluate_recommend_window(a, trY, emb, data_dir, trX=None):
    """--max_age HOURS: evaluate_recommend inside per-user candidate windows (see there)."""
    from dae_rnn_news_recommendation_amd import helpers
    from dae_rnn_news_recommendation_amd.synthetic import synthetic_timed_sessions
    K, n = a.recommend, emb.shape[0]
    assert trY is not None, "--sessions synthetic needs labels"
    seed = a.seed if a.seed >= 0 else 1234
    indptr, items, t, publish = synthetic_timed_sessions(max(n // 2, 1), np.unique(np.asarray(trY), return_inverse=True)[1],
                                                         mean_len=12, seed=seed)
    lens = np.diff(indptr)
    users = lens.shape[0]
    has = lens >= 2
    last = np.maximum(indptr[1:] - 1, 0)
    targets = np.where(has, items[last], -1).astype(np.int64)
    keep = np.ones(items.shape[0], dtype=bool)
    keep[indptr[1:][lens >= 1] - 1] = False                               # the history is everything before the last click
    h_ptr = np.zeros(users + 1, dtype=np.int64)
    h_ptr[1:] = np.cumsum(np.maximum(lens - 1, 0))
    hist = (h_ptr, items[keep])
    window = helpers.candidate_windows(t[last], publish, None if np.isinf(a.max_age) else a.max_age)
    mean_window = float((window[1] - window[0]).mean())
    states = helpers.user_states(hist, emb, a.session_decay, timestamps=t[keep], return_tensor=True)
    idx, score = helpers.recommend(states, emb, k=K, seen=hist, window=window)
    np.savez(data_dir + 'article_encoded_recommend%d_window.npz' % K, indices=idx, scores=score, targets=targets, window_lo=window[0],
             window_hi=window[1], max_age=a.max_age, mean_window=mean_window)
    m = helpers.next_click_metrics(idx, targets)
    b = helpers.next_click_metrics(helpers.popularity_recommend(hist, n, K, window=window), targets)
    print('  %d users, %d clicks, %d with a held-out click, max age %g h, mean window %.1f of %d articles -> '
          'article_encoded_recommend%d_window.npz' % (users, items.shape[0], m['n'], a.max_age, mean_window, n, K))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'decayed user state', m['hit'], m['mrr'], m['ndcg']))
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'most clicked unseen', b['hit'], b['mrr'], b['ndcg']))
    print('calculate recommend %d done' % K)
    if a.rec_dedup is not None:
        evaluate_recommend_dedup(a, states, emb, hist, targets, data_dir, window=window)
    if a.rec_mmr is not None:
        evaluate_recommend_mmr(a, trY, states, emb, hist, targets, data_dir, window=window)
    if a.covisit:
        evaluate_recommend_covisit(a, emb, hist, targets, data_dir, window=window)
    if a.als:
        evaluate_recommend_als(a, hist, targets, n, data_dir, window=window)
    if a.words:
        evaluate_recommend_words(a, trX, hist, targets, data_dir, window=window)
    models = {}
    if a.rank_metrics:
        evaluate_rank_metrics(states, emb, hist, targets, n, data_dir, window=window, max_age=a.max_age)
    if a.fit_user_model:
        models['fitted'] = evaluate_fitted_user_model(a, emb, hist, targets, n, data_dir, timestamps=t[keep], window=window)
    if a.user_model != 'decay':
        evaluate_recurrent_user_model(a, emb, hist, targets, n, data_dir, window=window, models=models)
    if a.every_click:
        evaluate_every_click(a, emb, (indptr, items), t, publish, models, data_dir)
    return idx, score, targets


def evaluate_fitted_user_model(a, emb, hist, targets, n, data_dir, timestamps=None, window=None):
    """--fit_user_model: the scaling vector alpha and the decay beta of the user model are learned from the histories the unfitted
    states were built from -- the held-out click is not among them -- by helpers.fit_user_model (negatives drawn uniformly over
    the corpus), saved as ``alpha`` / ``beta`` / ``history`` in user_model.npz, and the metrics of --recommend (and of
    --rank_metrics) are printed once more for ``alpha * state``; with ``window`` inside the same candidate windows."""
    from dae_rnn_news_recommendation_amd import helpers
    K = a.recommend
    print('fit user model')
    seed = a.seed if a.seed >= 0 else 1234
    model = helpers.fit_user_model(hist, emb, beta0=a.session_decay, seed=seed, timestamps=timestamps)
    np.savez(data_dir + 'user_model.npz', alpha=model.alpha, beta=model.beta, history=model.history)
    print('  %d steps, loss per pair %.4f -> %.4f, beta %.4f -> %.4f, alpha %.3f .. %.3f -> user_model.npz'
          % (model.history.size, model.history[0] if model.history.size else float('nan'),
             model.history[-1] if model.history.size else float('nan'), a.session_decay, model.beta, model.alpha.min(), model.alpha.max()))
    states = model.states(hist, emb, timestamps=timestamps, return_tensor=True)
    idx, _ = helpers.recommend(states, emb, k=K, seen=hist, window=window)
    m = helpers.next_click_metrics(idx, targets)
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f' % (K, 'fitted user model', m['hit'], m['mrr'], m['ndcg']))
    if a.rank_metrics:
        rank, _, n_cand = helpers.recommend_ranks(states, emb, targets, seen=hist, window=window)
        m = helpers.rank_metrics(rank, n_cand, targets, ks=(1, 10, 100))
        print('  ranks %-20s AUC %.4f  MRR %.4f  mean rank %.1f  median rank %.1f  hit@1 %.4f  hit@10 %.4f  hit@100 %.4f'
              % ('fitted user model', m['auc'], m['mrr'], m['mean_rank'], m['median_rank'], m['hit@1'], m['hit@10'], m['hit@100']))
    print('fit user model done')
    return model


def evaluate_recurrent_user_model(a, emb, hist, targets, n, data_dir, window=None, models=None):
    """--user_model gru: the recurrent user model on the histories the decayed states were built from.  The states come from
    helpers.gru_user_states with the weights of --gru_weights (helpers.GRUUserModel) -- or, with --fit_gru, with weights trained
    here by helpers.fit_gru_user_model on these histories and saved as gru_user_model.npz -- and go through the same helpers.recommend
    and, with --rank_metrics, helpers.recommend_ranks -- with ``window`` (--max_age) inside the same candidate windows.  The
    files are those of the decay model with `_gru` appended to the name: article_encoded_recommend{K}[_window]_gru.npz
    (``indices`` / ``scores`` / ``targets``) and article_encoded_ranks[_window]_gru.npz.  With --gru_validation FRACTION that share of
    the users (drawn by the fit's seed) is kept out of the fit and scored after every epoch by the every-click protocol
    (helpers.fit_gru_user_model(validation=...)).  ``models``: a dict that receives the model under 'gru' (for --every_click).
    --user_model lstm / rnn: the same path with helpers.lstm_user_states / helpers.rnn_user_states on the weights of --user_weights
    (helpers.LSTMUserModel / helpers.RNNUserModel) -- or, with --fit_cell, with weights trained here by helpers.fit_lstm_user_model /
    helpers.fit_rnn_user_model (--cell_epochs, --cell_validation) and saved as lstm_user_model.npz / rnn_user_model.npz --, `_lstm` /
    `_rnn` in the file names, the model under 'lstm' / 'rnn' in ``models``."""
    from dae_rnn_news_recommendation_amd import helpers
    K = a.recommend
    cell = a.user_model
    print('%s user model' % cell)
    if cell == 'gru':
        model = helpers.GRUUserModel.load(a.gru_weights) if a.gru_weights else None
    else:
        model = {'lstm': helpers.LSTMUserModel, 'rnn': helpers.RNNUserModel}[cell].load(a.user_weights) if a.user_weights else None
    if a.fit_gru or a.fit_cell:
        fit = {'gru': helpers.fit_gru_user_model, 'lstm': helpers.fit_lstm_user_model, 'rnn': helpers.fit_rnn_user_model}[cell]
        epochs, fraction = (a.gru_epochs, a.gru_validation) if a.fit_gru else (a.cell_epochs, a.cell_validation)
        seed = a.seed if a.seed >= 0 else 1234
        if fraction > 0:
            held = np.random.default_rng(seed).random(hist[0].size - 1) < fraction
            val = helpers.permute_histories(hist[0], hist[1], np.flatnonzero(held))
            model = fit(helpers.permute_histories(hist[0], hist[1], np.flatnonzero(~held)), emb, epochs=epochs, seed=seed, init=model,
                        validation=val)
        else:
            model = fit(hist, emb, epochs=epochs, seed=seed, init=model)
        for ep, v in enumerate(model.history):
            print('  fit epoch %d: loss per pair %.4f' % (ep + 1, v))
        for m in model.validation or ():
            print('  fit epoch %d: validation MRR %.4f  hit@10 %.4f  (%d clicks of %d held-out users)'
                  % (m['epoch'], m['mrr'], m['hit@10'], m['n'], int(held.sum())))
        model.save(data_dir + '%s_user_model.npz' % cell)
        print('  -> %s_user_model.npz' % cell)
    if models is not None:
        models[cell] = model
    assert model.input_size == emb.shape[1] and model.hidden_size == emb.shape[1], \
        "--%s_weights: input and hidden size (%d, %d) must equal the embedding size %d" \
        % ('gru' if cell == 'gru' else 'user', model.input_size, model.hidden_size, emb.shape[1])
    w = '' if window is None else '_window'
    states = model.states(hist, emb, return_tensor=True)
    idx, score = helpers.recommend(states, emb, k=K, seen=hist, window=window)
    np.savez(data_dir + 'article_encoded_recommend%d%s_%s.npz' % (K, w, cell), indices=idx, scores=score, targets=targets)
    m = helpers.next_click_metrics(idx, targets)
    print('  hit@%d %-20s %.4f  MRR %.4f  nDCG %.4f  -> article_encoded_recommend%d%s_%s.npz'
          % (K, cell + ' user state', m['hit'], m['mrr'], m['ndcg'], K, w, cell))
    if a.rank_metrics:
        rank, rscore, n_cand = helpers.recommend_ranks(states, emb, targets, seen=hist, window=window)
        np.savez(data_dir + 'article_encoded_ranks%s_%s.npz' % (w, cell), rank=rank, score=rscore, n_candidates=n_cand, targets=targets)
        m = helpers.rank_metrics(rank, n_cand, targets, ks=(1, 10, 100))
        print('  ranks %-20s AUC %.4f  MRR %.4f  mean rank %.1f  median rank %.1f  hit@1 %.4f  hit@10 %.4f  hit@100 %.4f'
              % (cell + ' user state', m['auc'], m['mrr'], m['mean_rank'], m['median_rank'], m['hit@1'], m['hit@10'], m['hit@100']))
    print('%s user model done' % cell)
    return idx, score


def evaluate_every_click(a, emb, sessions, t, publish, models, data_dir):
    """--every_click: next-click evaluation at every click of every session (helpers.evaluate_every_click), beside the last-click
    evaluation.  The state after each click is ranked against the click that follows among the articles the user had not
    clicked by then -- for the decay model (--session_decay), for the fitted and the GRU model when they were selected (``models``:
    fitted here on the sessions without their last click), and for the most-clicked-unseen baseline
    (helpers.popularity_ranks_every_click).  One line of rank metrics per model, then the MRR by clicks seen
    (helpers.rank_metrics_by_position).  Files: article_encoded_every_click[_fitted|_gru|_lstm|_rnn][_window].npz with ``rank`` / ``score`` /
    ``n_candidates`` / ``targets`` / ``positions``.  With ``publish`` (--max_age) every click competes only with the articles
    published by the time of the next click and at most --max_age hours before it."""
    from dae_rnn_news_recommendation_amd import helpers
    print('calculate every click')
    n = emb.shape[0]
    window, w = None, ''
    if publish is not None:
        times = helpers.every_click_rows(sessions, t)['query_times']
        window, w = helpers.candidate_windows(times, publish, None if np.isinf(a.max_age) else a.max_age), '_window'
    runs = [('decayed user state', '', a.session_decay)]
    if 'fitted' in models:
        runs.append(('fitted user model', '_fitted', models['fitted']))
    for cell in ('gru', 'lstm', 'rnn'):
        if cell in models:
            runs.append((cell + ' user state', '_' + cell, models[cell]))
    rows = []
    for name, tag, model in runs:
        r = helpers.evaluate_every_click(sessions, emb, model, timestamps=t, window=window, ks=(1, 10, 100))
        np.savez(data_dir + 'article_encoded_every_click%s%s.npz' % (tag, w), rank=r['rank'], score=r['score'],
                 n_candidates=r['n_candidates'], targets=r['targets'], positions=r['positions'])
        rows.append((name, r['metrics'], helpers.rank_metrics_by_position(r['rank'], r['n_candidates'], r['targets'], r['positions'], ks=())))
    b_rank, b_cand, targets = helpers.popularity_ranks_every_click(sessions, n, window=window)
    positions = helpers.every_click_rows(sessions)['positions']
    rows.append(('most clicked unseen', helpers.rank_metrics(b_rank, b_cand, targets, ks=(1, 10, 100)),
                 helpers.rank_metrics_by_position(b_rank, b_cand, targets, positions, ks=())))
    print('  %d users, %d clicks, %d with a next click -> article_encoded_every_click%s.npz'
          % (sessions[0].shape[0] - 1, sessions[1].shape[0], rows[0][1]['n'], w))
    for name, m, _ in rows:
        print('  every click %-20s AUC %.4f  MRR %.4f  mean rank %.1f  median rank %.1f  hit@1 %.4f  hit@10 %.4f  hit@100 %.4f'
              % (name, m['auc'], m['mrr'], m['mean_rank'], m['median_rank'], m['hit@1'], m['hit@10'], m['hit@100']))
    print('  MRR by clicks seen %s' % ''.join('  %20s' % name for name, _, _ in rows))
    for i, bucket in enumerate(rows[0][2]):
        span = '%d+' % bucket['lo'] if bucket['hi'] is None else ('%d' % bucket['lo'] if bucket['hi'] == bucket['lo'] + 1
                                                                  else '%d-%d' % (bucket['lo'], bucket['hi'] - 1))
        print('  seen %-6s n %6d %s' % (span, bucket['n'], ''.join('  %20.4f' % by[i]['mrr'] for _, _, by in rows)))
    print('calculate every click done')
    return rows


def evaluate_rank_metrics(states, emb, hist, targets, n, data_dir, window=None, max_age=0.):
    """--rank_metrics: the rank of every held-out click among all the articles the user has not read (helpers.recommend_ranks:
    no users x articles matrix), saved as ``rank`` / ``score`` / ``n_candidates`` / ``targets`` in article_encoded_ranks.npz, and
    one line per model -- the decayed user state and the most-clicked-unseen baseline (host code) -- with AUC, untruncated
    MRR, mean / median rank and hit@{1, 10, 100}.  With ``window`` (--max_age) both models rank inside the users' candidate
    windows and the file is article_encoded_ranks_window.npz, with the window's parameters."""
    from dae_rnn_news_recommendation_amd import helpers
    print('calculate rank metrics')
    if window is not None:
        rank, score, n_cand = helpers.recommend_ranks(states, emb, targets, seen=hist, window=window)
        np.savez(data_dir + 'article_encoded_ranks_window.npz', rank=rank, score=score, n_candidates=n_cand, targets=targets,
                 window_lo=window[0], window_hi=window[1], max_age=max_age, mean_window=float((window[1] - window[0]).mean()))
        b_rank, b_cand = helpers.popularity_ranks(hist, n, targets, window=window)
        for name, m in (('decayed user state', helpers.rank_metrics(rank, n_cand, targets, ks=(1, 10, 100))),
                        ('most clicked unseen', helpers.rank_metrics(b_rank, b_cand, targets, ks=(1, 10, 100)))):
            print('  ranks %-20s AUC %.4f  MRR %.4f  mean rank %.1f  median rank %.1f  hit@1 %.4f  hit@10 %.4f  hit@100 %.4f'
                  % (name, m['auc'], m['mrr'], m['mean_rank'], m['median_rank'], m['hit@1'], m['hit@10'], m['hit@100']))
        print('calculate rank metrics done -> article_encoded_ranks_window.npz')
        return
    rank, score, n_cand = helpers.recommend_ranks(states, emb, targets, seen=hist)
    np.savez(data_dir + 'article_encoded_ranks.npz', rank=rank, score=score, n_candidates=n_cand, targets=targets)
    b_rank, b_cand = helpers.popularity_ranks(hist, n, targets)
    for name, m in (('decayed user state', helpers.rank_metrics(rank, n_cand, targets, ks=(1, 10, 100))),
                    ('most clicked unseen', helpers.rank_metrics(b_rank, b_cand, targets, ks=(1, 10, 100)))):
        print('  ranks %-20s AUC %.4f  MRR %.4f  mean rank %.1f  median rank %.1f  hit@1 %.4f  hit@10 %.4f  hit@100 %.4f'
              % (name, m['auc'], m['mrr'], m['mean_rank'], m['median_rank'], m['hit@1'], m['hit@10'], m['hit@100']))
    print('calculate rank metrics done -> article_encoded_ranks.npz')


# artefact names of the reference's data directory (main_autoencoder.py:227-244, restored at :162-174)
def _artefact(kind, a, validate=False):
    suffix = "_validate" if validate else ""
    if kind == "features":
        stem = "article_tfidf_vectorized" if a.input_format == "tfidf" else "article_binary_count_vectorized"
        return stem + suffix + ".npz"
    return "article_label_" + a.label + suffix + ".pkl"


def vectorize_data(a, data_dir, helpers):
    """--vectorize: ``--data`` is a RAW count matrix (scipy .npz; rows = articles, columns = the whole vocabulary), and the stage
    the reference runs in front of training (:206-240) runs on the device (helpers.vectorize).  The first ``train_row`` rows fit the
    vocabulary -- ``CountVectorizer``'s ``min_df`` / ``max_df`` / ``max_features`` rule on the count matrix (helpers.limit_features) --
    and the idf (helpers.TfidfTransformer); the validation rows go through both.  With ``data_dir`` the count, binary and tf-idf
    matrices are saved under the reference's names (:233-240), with the kept columns (vocabulary_kept.npy) and the fitted
    transformer (tfidf_transformer.npz) where the reference pickles its two sklearn objects.  Returns the matrices
    ``--input_format`` selects and the labels.  The matrices come back as host scipy copies -- the artefacts are saved from them, and
    the estimator's ``fit`` / ``transform`` and the evaluation steps take host matrices -- so the CLI uploads the chosen one once more
    for training; a caller that wants no round trip hands ``return_device=True`` results to ``Engine.upload_csr`` itself."""
    assert a.data.endswith(".npz"), "--vectorize needs --data <counts.npz>, a scipy sparse count matrix"
    from dae_rnn_news_recommendation_amd.engine import Engine
    n = a.train_row + (a.validate_row if a.validation else 0)
    X = sparse.load_npz(a.data).tocsr()[:n]
    y = np.load(a.labels, allow_pickle=True)[:n] if a.labels else None
    n_train = min(a.train_row, X.shape[0])
    parts = [('', Engine.to_device_csr(X[:n_train], 'cuda'))]
    if a.validation and X.shape[0] > n_train:
        parts.append(('_validate', Engine.to_device_csr(X[n_train:], 'cuda')))
    counts, kept = helpers.limit_features(parts[0][1], a.min_df, a.max_df, a.max_features, return_device=True)
    tfidf = helpers.TfidfTransformer().fit(counts)
    out = {}
    for suffix, raw in parts:
        c = counts if suffix == '' else helpers.select_columns(raw, kept, return_device=True)
        forms = {'count': helpers.device_csr_to_scipy(c)}
        forms['binary_count'] = helpers.binarize(forms['count'])
        forms['tfidf'] = tfidf.transform(c)
        out[suffix] = forms['tfidf' if a.input_format == 'tfidf' else 'binary_count']
        if data_dir is not None:
            for stem, M in forms.items():
                helpers.save_file(M, data_dir + 'article_' + stem + '_vectorized' + suffix + '.npz')
    if data_dir is not None:
        np.save(data_dir + 'vocabulary_kept.npy', kept)
        tfidf.save(data_dir + 'tfidf_transformer.npz')
    print('vectorize: %d of %d columns kept, fitted on %d rows' % (kept.size, X.shape[1], n_train))
    trY = None if y is None else np.asarray(y[:n_train])
    vlY = None if (y is None or '_validate' not in out) else np.asarray(y[n_train:])
    return out[''], out.get('_validate'), trY, vlY


def load_or_restore(a, data_dir, helpers):
    """Train / validation matrices and label vectors: restored from the model's data directory
    (``--restore_previous_data``, reference :161-174) or built by ``load_data`` and saved there under the reference's
    artefact names and formats (scipy .npz for the vectorised text, pickled pandas Series for the labels, :227-240)."""
    import pandas as pd
    if a.restore_previous_data:
        trX = helpers.read_file(data_dir + _artefact("features", a))
        vlX = helpers.read_file(data_dir + _artefact("features", a, True)) if a.validation else None
        trY = helpers.read_file(data_dir + _artefact("label", a), data_type='pandas_series').to_numpy()
        vlY = helpers.read_file(data_dir + _artefact("label", a, True), data_type='pandas_series').to_numpy() if a.validation else None
        return trX, vlX, trY, vlY
    from dae_rnn_news_recommendation_amd import dp
    if a.vectorize:
        trX, vlX, trY, vlY = vectorize_data(a, data_dir if dp.rank() == 0 else None, helpers)
    else:
        X, y = load_data(a)
        trX, vlX = X[:a.train_row], (X[a.train_row:a.train_row + a.validate_row] if a.validation else None)
        trY = None if y is None else np.asarray(y[:a.train_row])
        vlY = None if (y is None or not a.validation) else np.asarray(y[a.train_row:a.train_row + a.validate_row])
    if dp.rank() != 0:                     # data parallel: rank 0 is the only writer of the shared artefact directory
        return trX, vlX, trY, vlY
    for M, val in ((trX, False), (vlX, True)):
        if M is not None and not a.vectorize:                           # vectorize_data has saved all three forms
            helpers.save_file(M if sparse.issparse(M) else np.asarray(M), data_dir + (_artefact("features", a, val) if sparse.issparse(M)
                              else _artefact("features", a, val).replace(".npz", ".npy")))
    for v, val in ((trY, False), (vlY, True)):
        if v is not None:
            helpers.save_file(pd.Series(v, name="label_" + a.label), data_dir + _artefact("label", a, val))
    return trX, vlX, trY, vlY


def main(argv=None):
    a = validate(build_parser().parse_args(argv))
    print(__file__ + ': Start')
    from dae_rnn_news_recommendation_amd import dp
    from dae_rnn_news_recommendation_amd.autoencoder import DenoisingAutoencoder, utils
    if a.data_parallel:
        dp.init_from_env()
    model = DenoisingAutoencoder(
        model_name=a.model_name, main_dir=a.main_dir, compress_factor=a.compress_factor, enc_act_func=a.enc_act_func,
        dec_act_func=a.dec_act_func, loss_func=a.loss_func, num_epochs=a.num_epochs, batch_size=a.batch_size,
        xavier_init=a.xavier_init, opt=a.opt, learning_rate=a.learning_rate, momentum=a.momentum, corr_type=a.corr_type,
        corr_frac=a.corr_frac, verbose=a.verbose, verbose_step=a.verbose_step, seed=a.seed, alpha=a.alpha,
        triplet_strategy=a.triplet_strategy, precision=a.precision, rng=a.rng, data_parallel=a.data_parallel)
    from dae_rnn_news_recommendation_amd import helpers
    trX, vlX, trY, vlY = load_or_restore(a, model.data_dir, helpers)
    need_labels = a.triplet_strategy != 'none'
    model.fit(trX, vlX, trY if need_labels else None, vlY if need_labels else None,
              restore_previous_model=a.restore_previous_model)
    if dp.rank() == 0:
        with open(model.parameter_file, 'a+') as fh:                    # reference :279-285
            print('train_row={}'.format(a.train_row), file=fh)
            print('validate_row={}'.format(a.validate_row), file=fh)
            print('input_format={}'.format(a.input_format), file=fh)
            print('label={}'.format(a.label), file=fh)
    # encode with the decay compensation the reference applies at inference (:289-290)
    emb = model.transform(utils.decay_noise(trX, a.corr_frac), name='article_encoded_train', save=True)
    emb_v = None
    if vlX is not None:
        emb_v = model.transform(utils.decay_noise(vlX, a.corr_frac), name='article_encoded_validate', save=True)
    if a.save_tsv and dp.rank() == 0:                                  # TensorBoard-projector exports (reference :293-303)
        import pandas as pd
        helpers.save_file(np.asarray(emb), model.tsv_dir + 'article_encoded.tsv')
        if emb_v is not None:
            helpers.save_file(np.asarray(emb_v), model.tsv_dir + 'article_encoded_validate.tsv')
        if trY is not None:
            helpers.save_file(pd.DataFrame({'label_' + a.label: trY}), model.tsv_dir + 'article_label.tsv')
        if vlY is not None:
            helpers.save_file(pd.DataFrame({'label_' + a.label: vlY}), model.tsv_dir + 'article_label_validate.tsv')
    if a.similarity and dp.rank() == 0:
        evaluate_similarity(a, trX, vlX, trY, vlY, emb, emb_v, model.plot_dir)
    if a.label_stats and dp.rank() == 0:
        evaluate_label_stats(a, trX, vlX, trY, vlY, emb, emb_v, model.plot_dir)
    if a.top_k > 0 and dp.rank() == 0:
        evaluate_top_k(a, trX, vlX, trY, vlY, emb, emb_v, model.data_dir)
    if a.dup_threshold > 0 and dp.rank() == 0:
        evaluate_duplicates(a, trY, vlY, emb, emb_v, model.data_dir)
    if a.cluster > 0 and dp.rank() == 0:
        evaluate_clusters(a, trY, vlY, emb, emb_v, model.data_dir)
    if a.recommend > 0 and dp.rank() == 0:
        evaluate_recommend(a, trY, emb, model.data_dir, trX)
    if model.samples_per_sec:
        print('training throughput: %.0f samples/s over %d epochs; embeddings %s -> %s' %
              (model.samples_per_sec, a.num_epochs, emb.shape, model.data_dir))
    print(__file__ + ': End')
    return model


if __name__ == '__main__':
    main()
