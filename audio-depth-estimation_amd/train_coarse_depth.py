"""MI355X counterpart of /root/reference/train_coarse_depth.py: same flags, same loop, fused libadn steps (train_dc.py).

    python -m audio_depth_estimation_amd.train_coarse_depth --synthetic 64 --epochs 1 --batch_size 8 --graph
"""
from .train_dc import main_coarse as main

if __name__ == '__main__':
    main()
