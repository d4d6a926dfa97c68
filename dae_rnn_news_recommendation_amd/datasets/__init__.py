"""Mirror of the functions of the reference's ``datasets`` package the training paths need: ``similar_articles`` (host code, the
explicit-triplet path) and ``tfidf_transform`` (the count matrix to tf-idf, on the device)."""
from .articles import similar_articles, tfidf_transform  # noqa: F401
