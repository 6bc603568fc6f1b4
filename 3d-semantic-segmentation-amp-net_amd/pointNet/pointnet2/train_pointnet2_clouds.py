#!/usr/bin/env python3
"""CLI of the PointNet++ segmentation model's training driver on clusters of NATIVE size (pointNet/pn2_train.py: train_pn2_clouds) on the
HIP path, in the form of train_pointnet2_segmen.py: it trains on the `<name>_clusters_list.pkl` files infer_pointnet2_segmen.py
evaluates, shuffled and rotated on the device.  The reference has no such file.  The model is exact fp32, so there is no --precision flag.
Run from the repository root:  python <package>/pointNet/pointnet2/train_pointnet2_clouds.py --cluster_dir k_means_25 ..."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--cluster_dir', type=str, default='k_means_25')
    parser.add_argument('--path_list_files', type=str, default='train_test_files/RGBN_100x100_old/RGBN_100x100_kmeans')
    parser.add_argument('--output_folder', type=str, default='pointNet/results')
    parser.add_argument('--files_per_step', type=int, default=16)
    parser.add_argument('--epochs', type=int, default=500)
    parser.add_argument('--learning_rate', type=float, default=0.0005)
    parser.add_argument('--number_of_workers', type=int, default=4)
    parser.add_argument('--model_checkpoint', type=str, default='')
    parser.add_argument('--seed', type=lambda v: int(v, 0), default=0x6A09E667, help='seed of the device augmentation (decimal or 0x...)')
    parser.add_argument('--device', type=str, default='cuda')
    return parser


def main(argv=None):
    a = build_parser().parse_args(argv)
    train = importlib.import_module("3d-semantic-segmentation-amp-net_amd.pointNet.pn2_train").train_pn2_clouds
    return train(a.cluster_dir, a.path_list_files, a.output_folder, a.files_per_step, a.epochs, a.learning_rate, a.number_of_workers,
                 a.model_checkpoint, a.device, seed=a.seed)


if __name__ == '__main__':
    main()
