"""Target generation: the reference's `tasks/` scripts as library code."""
