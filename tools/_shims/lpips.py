"""Stand-in for lpips: the reference's eval/calc_metrics.py imports it at the top and uses it in its map step only."""
