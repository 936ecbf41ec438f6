"""MI355X (gfx950) path of the NCF models.  The recommendation functions are re-exported here, imported on first use."""
_RECOMMEND = ("top_k_items", "recommend_for_user", "seen_items")


def __getattr__(name):
    if name in _RECOMMEND:
        from . import recommend
        return getattr(recommend, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
