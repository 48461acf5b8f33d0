def build_tail_model(*args, **kwargs):
    """tksm_amd.sequence.build_tail_model (imported on first use: importing the package loads nothing)"""
    from .sequence import build_tail_model as f
    return f(*args, **kwargs)
