"""Stand-in for skimage: the reference's eval/calc_metrics.py imports skimage.measure at the top and uses it in its map step only."""
