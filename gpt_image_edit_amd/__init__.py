__all__ = ["edit_region_weights"]


def __getattr__(name):
    # resolved on first use, so importing the package stays as light as it was
    if name == "edit_region_weights":
        from .edit_weights import edit_region_weights
        return edit_region_weights
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
