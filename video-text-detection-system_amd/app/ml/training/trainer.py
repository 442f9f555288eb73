"""app.ml.training.trainer (reference: app/ml/training/trainer.py) -> MI355X implementation: the loss (forward and analytic backward),
the validation metrics, the opt-in HIP AdamW step and the trainer surface (TextDetectionLightningModule as a plain nn.Module;
ModelTrainer is a stub)."""
from vtd_amd.training import (AdamW, BinaryMetricCounts, DiceLoss, ModelTrainer, TextDetectionDataset, TextDetectionLightningModule,  # noqa: F401
                              detection_loss, precision_recall_f1)
