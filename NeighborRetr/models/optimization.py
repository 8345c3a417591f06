"""`NeighborRetr.models.optimization` of the reference (optimization.py:17-211) -> neighborretr_amd.optim."""
from neighborretr_amd.optim import SCHEDULES, BertAdam, warmup_constant, warmup_cosine, warmup_linear  # noqa: F401
