"""The training-time callback group of experiment=play_lmp_for_rl (reference config/callbacks/play_lmp.yaml: kl_schedule,
tsne_plot) under the reference's module paths."""
