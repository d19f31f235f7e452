"""Training on the GPU: the hardest-contrastive loss (loss.py), the 3DMatch pair data set and collate (data.py), the
trainer and its command line (trainer.py, `python -m imfnet_amd.train`)."""
