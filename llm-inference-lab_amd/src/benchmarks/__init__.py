"""Quality tools over the HIP models (the reference's `src.benchmarks`)."""
