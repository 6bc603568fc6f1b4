#!/usr/bin/env python3
"""test_pointnet2_segmen.py on precomputed clusters: the same flags and defaults plus --cluster_dir and --files_per_launch, the work is
pn2_infer.test (all clusters of a file, or of several files, as ONE ragged launch sequence; the metrics counted on the device).  The model is
exact fp32, so there is no --precision flag."""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--dataset_path', type=str, default='/dades/LIDAR/towers_detection/datasets/towers_100x100')
    parser.add_argument('--out_path', type=str, default='results')
    parser.add_argument('--number_of_points', type=int, default=2048)
    parser.add_argument('--number_of_workers', type=int, default=0)
    parser.add_argument('--model_checkpoint', type=str, default='')
    parser.add_argument('--path_list_files', type=str, default='train_test_files/RGBN_100x100_old')
    parser.add_argument('--device', type=str, default='cuda')
    parser.add_argument('--cluster_dir', type=str, default='k_means_25')
    parser.add_argument('--files_per_launch', type=int, default=1, help='files that share one launch sequence; the metrics do not depend on it')
    return parser


def main(argv=None):
    a = build_parser().parse_args(argv)
    test = importlib.import_module("3d-semantic-segmentation-amp-net_amd.pointNet.pn2_infer").test
    return test(a.dataset_path, a.out_path, a.number_of_points, a.number_of_workers, a.model_checkpoint, a.path_list_files, a.cluster_dir,
                a.device, files_per_launch=a.files_per_launch)


if __name__ == '__main__':
    main()
