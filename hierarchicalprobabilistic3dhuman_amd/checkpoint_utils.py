"""utils/checkpoint_utils.py: what the training loop reads from a checkpoint it resumes from."""
import numpy as np


def load_training_info_from_checkpoint(checkpoint, save_val_metrics):
    """utils/checkpoint_utils.py:4-26 -> (current_epoch, best_epoch, best_model_wts, best_epoch_val_metrics).  ``checkpoint``: the dict
    the loop saves ('epoch', 'best_epoch', 'best_model_state_dict', 'best_epoch_val_metrics', ...).  Training continues at the epoch
    after the saved one.  The best values are the checkpoint's own dict, edited in place as the reference edits it: a metric of
    ``save_val_metrics`` it does not hold starts at infinity, a metric it holds that is no longer asked for is dropped."""
    current_epoch = checkpoint['epoch'] + 1
    best_epoch = checkpoint['best_epoch']
    best_epoch_val_metrics = checkpoint['best_epoch_val_metrics']
    for metric in save_val_metrics:
        best_epoch_val_metrics.setdefault(metric, np.inf)
    for metric in [m for m in best_epoch_val_metrics if m not in save_val_metrics]:
        del best_epoch_val_metrics[metric]
    print('\nTraining information loaded from checkpoint.')
    print('Current epoch:', current_epoch)
    print('Best epoch val metrics from last training run:', best_epoch_val_metrics, ' - achieved in epoch:', best_epoch)
    return current_epoch, best_epoch, checkpoint['best_model_state_dict'], best_epoch_val_metrics
