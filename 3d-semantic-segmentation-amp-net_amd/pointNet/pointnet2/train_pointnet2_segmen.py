#!/usr/bin/env python3
"""CLI of the PointNet++ segmentation model's training driver (pointNet/pn2_train.py: train_pn2) on the HIP path, in the form of
pointNet/rnn/train_pointnetGRU.py.  The reference has no such file: its pointnet_2 carries the classifier commented out.  The model is
exact fp32, so there is no --precision flag.
Run from the repository root:  python <package>/pointNet/pointnet2/train_pointnet2_segmen.py --dataset_path DATASET ..."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataset_path', type=str, default='/dades/LIDAR/towers_detection/datasets/kmeans_100x100c9_2048')
    parser.add_argument('--path_list_files', type=str, default='train_test_files/RGBN_100x100_old/RGBN_100x100_kmeans')
    parser.add_argument('--output_folder', type=str, default='pointNet/results')
    parser.add_argument('--number_of_points', type=int, default=2048)
    parser.add_argument('--batch_size', type=int, default=32)
    parser.add_argument('--epochs', type=int, default=500)
    parser.add_argument('--learning_rate', type=float, default=0.0005)
    parser.add_argument('--number_of_workers', type=int, default=4)
    parser.add_argument('--model_checkpoint', type=str, default='')
    parser.add_argument('--device', type=str, default='cuda')
    return parser


def main(argv=None):
    a = build_parser().parse_args(argv)
    train_pn2 = importlib.import_module("3d-semantic-segmentation-amp-net_amd.pointNet.pn2_train").train_pn2
    return train_pn2(a.dataset_path, a.path_list_files, a.output_folder, a.number_of_points, a.batch_size, a.epochs, a.learning_rate,
                     a.number_of_workers, a.model_checkpoint, a.device)


if __name__ == '__main__':
    main()
