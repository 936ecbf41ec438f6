"""MI355X (gfx950) path of the NCF models.  The recommendation and ranking-evaluation functions, the baselines and the
implicit-feedback protocol are re-exported here, imported on first use."""
_RECOMMEND = ("top_k_items", "recommend_for_user", "seen_items", "rated_exclusion", "explain_items", "content_cosine_top_k",
              "content_cosine_ranks", "attention_statistics", "attention_stat_ratios", "AttentionStats", "diversify_top_k", "item_vectors",
              "item_knn_top_k", "item_knn_ranks", "ease_top_k", "ease_ranks", "slim_top_k", "slim_ranks")
_RANKING_EVAL = ("rank_of_items", "ranking_metrics", "eval_full_ranking", "held_out_items", "intra_list_diversity", "catalogue_coverage")
_BASELINES = ("KernelMF", "ItemKNN", "ImplicitALS", "EASE", "SLIM")
_IMPLICIT = ("leave_one_out", "ImplicitFeedback", "fit_implicit", "sampled_candidates", "eval_sampled", "rank_sampled")


def __getattr__(name):
    if name in _RECOMMEND:
        from . import recommend
        return getattr(recommend, name)
    if name in _RANKING_EVAL:
        from . import ranking_eval
        return getattr(ranking_eval, name)
    if name in _BASELINES:
        from . import baselines
        return getattr(baselines, name)
    if name in _IMPLICIT:
        from . import implicit
        return getattr(implicit, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
