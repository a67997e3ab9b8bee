"""furnace/tools: the benchmark helpers the `.speed` experiments import (`from tools.benchmark import compute_speed,
stat`)."""
