"""`NeighborRetr.training.optimizer` of the reference (optimizer.py:12-86) -> neighborretr_amd.optim."""
from neighborretr_amd.optim import prep_optimizer  # noqa: F401
