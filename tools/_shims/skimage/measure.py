"""Stand-in for skimage.measure: nothing of it runs under --reduce_only."""
