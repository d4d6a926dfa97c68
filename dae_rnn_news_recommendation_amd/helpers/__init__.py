"""Mirror of the parts of the reference's ``helpers.py`` either side of the training path, and what grew around them.  Every name
is importable from here; the code lives by subject:

* ``io`` -- ``save_file`` / ``read_file`` (helpers.py:138-264): the on-disk artefact conventions.  Host code.
* ``sweeps`` -- ``pairwise_similarity`` (helpers.py:11-50; the evaluation step ``main_autoencoder.py:307-317`` runs six times right
  after training) and the sweeps by the same scores without the N x N matrix: ``most_similar`` (top-k; ``exclude``,
  ``exclude_shared``, ``window`` / ``candidate_windows``, ``chunk_rows=``, ``dedup_threshold=``), ``target_ranks`` (full rank of one
  target per row), ``similar_pairs`` (near-duplicate search), ``dedup_lists`` (greedy de-duplication of recommendation lists) and
  ``diversify_lists`` (MMR re-ranking of such lists for diversity, with a de-dup threshold and a cap per label); the ``normalize_*`` forms of the row filter; the chunk plan (``sweep_chunk_rows``, ``sweep_chunk_plan``, ``label_stats_blocks``)
  and ``SweepOperand``, one operand of a sweep in the form it came in.
* ``label_stats`` -- ``visualize_pairwise_similarity`` (helpers.py:79-135) and ``label_similarity_stats``, the same AUROC and box-plot
  numbers without the N x N matrix (``stats_from_histograms``); ``label_precision_at_k``, ``duplicate_groups`` and
  ``duplicate_pair_precision`` score a top-k or a near-duplicate result against labels.  Host code but for the first two.
* ``user_models`` -- the user models of "Embedding-based News Recommendation for Millions of Users": ``user_states`` (decaying;
  ``decay_factors``), ``fit_user_model`` / ``UserModel`` on ``user_pair_loss`` (``sample_negatives``,
  ``decay_factor_derivatives``); ``GRUUserModel``, ``gru_user_states`` (``gru_schedule``, ``trim_histories``),
  ``fit_gru_user_model`` on ``gru_pair_loss``; ``LSTMUserModel`` / ``lstm_user_states`` / ``fit_lstm_user_model`` on ``lstm_pair_loss``
  and ``RNNUserModel`` / ``rnn_user_states`` / ``fit_rnn_user_model`` on ``rnn_pair_loss``.
* ``evaluation`` -- ``recommend`` / ``recommend_ranks`` with ``next_click_metrics`` / ``rank_metrics``, ``recommend_diverse``
  (``recommend`` + ``diversify_lists``) with ``list_diversity`` (nearest similarity, labels per list), the popularity baseline
  (``popularity_recommend``, ``popularity_ranks``), and the every-click protocol (``click_prefix_lists``, ``every_click_rows``,
  ``recommend_every_click``, ``recommend_ranks_every_click``, ``evaluate_every_click``, ``rank_metrics_by_position``,
  ``popularity_ranks_every_click``).
* ``vectorize`` -- the stage in front of training (main_autoencoder.py:206-240) on a raw count matrix that stays on the device as
  CSR: ``column_stats`` (df and tf per column), ``limit_features`` / ``limit_features_columns`` / ``select_columns``
  (``CountVectorizer._limit_features``), ``TfidfTransformer`` (sklearn's, fitted on train, applied to validation), ``binarize``.
* ``clustering`` -- spherical k-means on the device (``kmeans`` -> ``KMeansResult``, ``kmeans_assign``, ``relocation_rows``),
  ``cluster_label_scores`` (purity / NMI / ARI against labels; host code) and ``ClusterIndex``, cluster-probed top-k on the windowed
  ``most_similar`` (``merge_probe_lists``).
* ``covisit`` -- the co-visitation baseline, built from co-clicks alone: ``covisit_neighbors`` -> ``CovisitIndex`` (``recommend``,
  ``similar``, ``save`` / ``load``), ``covisit_recommend``, ``fill_popular_tails`` and ``list_overlap`` (two neighbour tables
  compared; host code).
* ``als`` -- implicit-feedback matrix factorisation by alternating least squares, the ID-based collaborative filter:
  ``als_interactions`` -> ``ALSInteractions`` (both orientations of the click counts), ``als_gram``, ``als_solve_rows`` (one
  half-sweep of conjugate gradient per row), ``als_loss``, and ``fit_als`` -> ``ALSModel`` (``user_states``, ``recommend``,
  ``similar``, ``save`` / ``load``).
* ``words`` -- the paper's word-based baseline: ``word_profiles`` -> ``WordProfiles`` (the users' word sets as device bitmaps;
  ``to_scipy``), ``word_recommend`` (top-k of the weighted count of shared words, sparse on both sides), ``word_ranks`` (its
  full-rank twin, in the form ``rank_metrics`` takes) and ``idf_weights`` (sklearn's smooth idf as term weights).
* ``_device`` -- what every device call starts and ends with, once: device and library, the ``norm`` / ``metric`` check, the
  matrix and history intakes, uploads, workspaces, the result tail.

The device functions have no CPU implementation: without the built library / a GPU they raise.  torch, scipy and pandas are
imported inside the functions that need them; importing this package needs numpy alone."""
from .als import ALSInteractions, ALSModel, als_gram, als_interactions, als_loss, als_solve_rows, fit_als
from .clustering import (ClusterIndex, KMeansResult, cluster_label_scores, kmeans, kmeans_assign, merge_probe_lists,
                         relocation_rows)
from .covisit import CovisitIndex, covisit_neighbors, covisit_recommend, fill_popular_tails, list_overlap
from .evaluation import (click_prefix_lists, evaluate_every_click, every_click_rows, list_diversity, next_click_metrics,
                         popularity_ranks, popularity_ranks_every_click, popularity_recommend, rank_metrics, rank_metrics_by_position,
                         recommend, recommend_diverse, recommend_every_click, recommend_ranks, recommend_ranks_every_click)
from .io import read_file, save_file
from .label_stats import _STAT_KEYS  # noqa: F401  (the tests read it)
from .label_stats import (duplicate_groups, duplicate_pair_precision, label_precision_at_k, label_similarity_stats,
                          stats_from_histograms, visualize_pairwise_similarity)
from .sweeps import competitors as _competitors  # noqa: F401  (the tests call it by its earlier name)
from .sweeps import (SWEEP_AUTO_IMAGE_BYTES, SweepOperand, candidate_windows, dedup_lists, diversify_lists, label_stats_blocks, most_similar,
                     normalize_exclusions, normalize_shared_exclusions, normalize_window, pairwise_similarity, permute_histories,
                     shared_pairs, shared_row_chunks, similar_pairs, sweep_chunk_plan, sweep_chunk_rows, target_ranks)
from .user_models import (GRUUserModel, LSTMUserModel, RNNUserModel, UserModel, decay_factor_derivatives, decay_factors,
                          fit_gru_user_model, fit_lstm_user_model, fit_rnn_user_model, fit_user_model, gru_pair_loss, gru_schedule,
                          gru_user_states, lstm_pair_loss, lstm_user_states, rnn_pair_loss, rnn_user_states, sample_negatives,
                          trim_histories, user_pair_loss, user_states)
from .vectorize import (TfidfTransformer, binarize, column_stats, device_csr_to_scipy, limit_features, limit_features_columns,
                        select_columns)
from .words import WordProfiles, idf_weights, word_profiles, word_ranks, word_recommend
