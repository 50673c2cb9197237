from .cfgnode import CfgNode
from .metrics import mse2psnr, MSE, PSNR, SSIM, ssim_frames, estim_error, save_error
from .tensorf_utils import TVLoss, N_to_reso, mse_loss
from .evaluation_utils import save_checkpoint, load_checkpoint, load_model_checkpoint, render_test_evaluation, render_segm_evaluation, compute_depth_loss
from .ray_regs import distortion_loss, distortion_loss_raw
from .flow_loss import flow_loss_raw, flow_loss_backward_raw, flow_loss_plan
from .segm_utils import sample_volume_points, balanced_sample, segm_points
from .seg_loss import fit_motion_svd_batch, dynamic_loss, smooth_loss, entropy_loss, segm_losses
from .metric_segm import (eval_segm, accumulate_eval_results, calculate_AP, calculate_PQ_F1, ClusteringMetrics, SegmEvaluator, segm_confusion,
                          summary_from_confusion)
from .point_segm_util import compress_label, align_insts
