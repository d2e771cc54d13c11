"""The case table of the picked fp16 / fp32 GEMV tests (test_gemv_picked.py on the CPU, test_gpu_gemv_picked.py on the GPU), the
inputs of a case and its float64 reference.

launch_gemv chooses between two kernels and their template parameters with gemv_plan (kernels_gemv.hip); the test hook
nfai_hip_debug_gemv_plan runs that planner without a device.  A CLASS is what the planner can vary in the code that runs:

    (kernel, w_type, mode, norm, UPW | CH, U | RW, guard)      kernel 0 = k_gemv, 1 = k_gemv_sk; w_type 0 = fp32, 1 = fp16 (ggml);
                                                               mode 0 = PLAIN, 1 = RESIDUAL, 2 = q|k|v + RoPE, 3 = gate|up + SiLU

TABLE names, for every class the default pickers reach on 256 CUs below 128 MB of weights, at least one shape, with the launch
shape (threads per workgroup, grid) the planner gives it.  The shapes were found with the plan hook and are the smallest that reach
the class and still exercise its edges:

  k_gemv     NU % UPW != 0 (the last unit group is partial and its unit clamped) wherever the class allows it: NU = 1025, 2050,
             3073 leave most waves of the 256 workgroups without a group; a handful of rows (NU = 5..7 in two workgroups) for
             UPW = 1; GUARD forms at K = 8, 264 and 1000 (K % (64 EPL) small and large); every waves-per-workgroup value 4..8
             with and without the RMSNorm (the exact splits NU = 1280, 1536, 1792 and the K that no smaller workgroup holds);
             the three grid rules ceil(NU / 4), n_cu and 2 n_cu.  q|k|v goes through the ABI with whole heads of D = 64 / 128,
             so NU is a multiple of 32 there (96 = one q, one k, one v head of 64) and a partial last group exists for UPW = 3 only.
             PLAIN and RESIDUAL leave the split-K form only where K / (64 EPL) has no split into 2..16 waves (17 or 34 chunks:
             K = 8704 / 17408 fp16, 4352 / 8704 fp32; 21 = 3 * 7 chunks for U = 3), where the fused ArgMax would need more than
             1024 workgroups (NU > 4096), or above 256 MB.
  k_gemv_sk  three NU per class where the class allows them: below one workgroup (NU < RW / RPU), a partial last workgroup, an
             exact multiple; every wave count 2..16 with CH = 1 and 9..16 with CH = 2 and CH = 4, for both weight types.  RW = 16
             and RW = 8 need >= 60 MB of weights: 3840 x 8192 and 1920 x 16384 fp16 (exactly 60 MB) and one partial workgroup more;
             no NU below one workgroup exists there.

The last word of a row says whether the launch carries the fused ArgMax (nfai_hip_lmhead_argmax); PLAIN with the RMSNorm always
does, since that is the entry that passes gamma with PLAIN.
"""
import functools
from collections import namedtuple

import numpy as np

F32, F16 = 0, 1
PLAIN, RESIDUAL, QKV, GATEUP = 0, 1, 2, 3
MODE_NAMES = ["plain", "residual", "qkv", "gateup"]
N_CU = 256
CAP_BYTES = 128 << 20        # a class whose smallest shape is larger has no case (EXCLUDED)
EPS = 1e-5
GUARD = 8                    # sentinel elements behind every output
KV_CAP = 5                   # q|k|v: cache rows

# (kernel, w_type, mode, norm): [(UPW | CH, U | RW, guard, threads, grid, NU, K, fused ArgMax), ...]
TABLE = {
    (0, 0, 0, 0): [
        (1, 1, 0, 256, 2, 7, 256, 0), (1, 1, 0, 512, 2, 6, 28928, 0), (1, 1, 1, 256, 2, 5, 264, 0), (1, 1, 1, 256, 2, 6, 8, 0),
        (1, 1, 1, 256, 256, 1024, 8, 0), (1, 1, 1, 320, 256, 1280, 8, 0), (1, 1, 1, 384, 256, 1536, 8, 0),
        (1, 1, 1, 448, 256, 1792, 8, 0), (1, 2, 0, 256, 2, 7, 8704, 0), (1, 3, 0, 256, 2, 5, 5376, 0), (1, 4, 0, 320, 2, 6, 17408, 0),
        (2, 1, 0, 256, 256, 1025, 256, 0), (2, 1, 1, 256, 256, 1025, 1000, 0), (2, 2, 0, 256, 256, 1025, 8704, 0),
        (2, 3, 0, 256, 256, 1025, 5376, 0), (2, 4, 0, 320, 256, 1025, 17408, 0), (3, 1, 0, 256, 256, 2050, 256, 0),
        (3, 1, 1, 256, 256, 2050, 8, 0), (3, 2, 0, 256, 256, 2050, 8704, 0), (4, 1, 0, 256, 256, 3073, 256, 0),
        (4, 1, 1, 256, 256, 3073, 264, 0), (4, 2, 0, 256, 256, 3073, 8704, 0),
    ],
    (0, 0, 0, 1): [
        (1, 1, 0, 256, 2, 7, 256, 1), (1, 1, 0, 320, 2, 6, 4352, 1), (1, 1, 0, 448, 2, 7, 6400, 1), (1, 1, 0, 512, 2, 6, 7424, 1),
        (1, 1, 1, 256, 2, 6, 8, 1), (1, 1, 1, 256, 2, 7, 1000, 1), (1, 2, 0, 256, 256, 4097, 512, 1), (1, 3, 0, 384, 2, 5, 5376, 1),
        (1, 4, 0, 256, 256, 4097, 1024, 1), (2, 1, 0, 256, 256, 1025, 256, 1), (2, 1, 1, 256, 256, 1025, 8, 1),
        (2, 2, 0, 256, 256, 9217, 512, 1), (2, 3, 0, 384, 256, 1025, 5376, 1), (2, 4, 0, 256, 256, 5121, 1024, 1),
        (3, 1, 0, 256, 256, 2050, 256, 1), (3, 1, 1, 256, 256, 2050, 264, 1), (4, 1, 0, 256, 256, 3073, 256, 1),
        (4, 1, 1, 256, 256, 3073, 1000, 1), (4, 2, 0, 256, 256, 7169, 512, 1),
    ],
    (0, 0, 1, 0): [
        (1, 1, 0, 256, 2, 7, 256, 0), (1, 1, 1, 256, 2, 7, 1000, 0), (1, 2, 0, 256, 2, 7, 8704, 0), (1, 3, 0, 256, 2, 5, 5376, 0),
        (1, 4, 0, 320, 2, 6, 17408, 0), (2, 1, 0, 256, 256, 1025, 256, 0), (2, 1, 1, 256, 256, 1025, 8, 0),
        (2, 2, 0, 256, 256, 1025, 8704, 0), (2, 3, 0, 256, 256, 1025, 5376, 0), (2, 4, 0, 320, 256, 1025, 17408, 0),
        (3, 1, 0, 256, 256, 2050, 256, 0), (3, 1, 1, 256, 256, 2050, 264, 0), (3, 2, 0, 256, 256, 2050, 8704, 0),
        (4, 1, 0, 256, 256, 3073, 256, 0), (4, 1, 1, 256, 256, 3073, 1000, 0), (4, 2, 0, 256, 256, 3073, 8704, 0),
    ],
    (0, 0, 1, 1): [
        (1, 1, 0, 256, 2, 7, 256, 0), (1, 1, 1, 256, 2, 6, 8, 0), (1, 3, 0, 384, 2, 5, 5376, 0), (2, 1, 0, 256, 256, 1025, 256, 0),
        (2, 1, 1, 256, 256, 1025, 264, 0), (2, 3, 0, 384, 256, 1025, 5376, 0), (3, 1, 0, 256, 256, 2050, 256, 0),
        (3, 1, 1, 256, 256, 2050, 1000, 0), (4, 1, 0, 256, 256, 3073, 256, 0), (4, 1, 1, 256, 256, 3073, 8, 0),
    ],
    (0, 0, 2, 0): [
        (1, 1, 0, 256, 24, 96, 256, 0), (1, 1, 1, 256, 24, 96, 8, 0), (1, 1, 1, 256, 512, 2048, 8, 0), (1, 2, 0, 256, 24, 96, 512, 0),
        (1, 3, 0, 256, 24, 96, 768, 0), (1, 4, 0, 256, 24, 96, 1024, 0), (2, 1, 0, 256, 256, 1056, 256, 0),
        (2, 1, 1, 256, 256, 1056, 264, 0), (2, 2, 0, 256, 256, 1056, 512, 0), (3, 1, 0, 256, 512, 4160, 256, 0),
        (3, 1, 1, 256, 512, 4160, 1000, 0), (4, 1, 0, 256, 512, 8192, 256, 0), (4, 1, 1, 256, 512, 8192, 8, 0),
    ],
    (0, 0, 2, 1): [
        (1, 1, 0, 256, 24, 96, 256, 0), (1, 1, 1, 256, 24, 96, 264, 0), (1, 2, 0, 256, 24, 96, 512, 0), (1, 3, 0, 256, 24, 96, 768, 0),
        (1, 4, 0, 256, 24, 96, 1024, 0), (2, 1, 0, 256, 256, 1056, 256, 0), (2, 1, 1, 256, 256, 1056, 1000, 0),
        (2, 2, 0, 256, 256, 1056, 512, 0), (3, 1, 0, 256, 512, 4160, 256, 0), (3, 1, 1, 256, 512, 4160, 8, 0),
        (4, 1, 0, 256, 512, 8192, 256, 0), (4, 1, 1, 256, 512, 8192, 264, 0),
    ],
    (0, 0, 3, 0): [
        (1, 1, 0, 256, 2, 7, 256, 0), (1, 1, 1, 256, 2, 5, 264, 0), (1, 2, 0, 256, 2, 6, 512, 0), (1, 3, 0, 256, 2, 5, 768, 0),
        (1, 4, 0, 256, 2, 7, 1024, 0), (2, 1, 0, 256, 256, 1025, 256, 0), (2, 1, 1, 256, 256, 1025, 1000, 0),
        (2, 2, 0, 256, 256, 1025, 512, 0), (3, 1, 0, 256, 512, 4097, 256, 0), (3, 1, 1, 256, 512, 4097, 8, 0),
        (4, 1, 0, 256, 512, 6145, 256, 0), (4, 1, 1, 256, 512, 6145, 264, 0),
    ],
    (0, 0, 3, 1): [
        (1, 1, 0, 256, 2, 7, 256, 0), (1, 1, 1, 256, 2, 7, 1000, 0), (1, 2, 0, 256, 2, 6, 512, 0), (1, 3, 0, 256, 2, 5, 768, 0),
        (1, 4, 0, 256, 2, 7, 1024, 0), (2, 1, 0, 256, 256, 1025, 256, 0), (2, 1, 1, 256, 256, 1025, 8, 0),
        (2, 2, 0, 256, 256, 1025, 512, 0), (3, 1, 0, 256, 512, 4097, 256, 0), (3, 1, 1, 256, 512, 4097, 264, 0),
        (4, 1, 0, 256, 512, 6145, 256, 0), (4, 1, 1, 256, 512, 6145, 1000, 0),
    ],
    (0, 1, 0, 0): [
        (1, 1, 0, 256, 2, 6, 512, 0), (1, 1, 1, 256, 2, 6, 8, 0), (1, 1, 1, 256, 2, 7, 1000, 0), (1, 1, 1, 256, 256, 1024, 8, 0),
        (1, 1, 1, 320, 256, 1280, 8, 0), (1, 1, 1, 384, 256, 1536, 8, 0), (1, 1, 1, 448, 256, 1792, 8, 0),
        (1, 1, 1, 512, 2, 6, 28928, 0), (1, 2, 0, 320, 2, 6, 17408, 0), (1, 3, 0, 256, 2, 5, 10752, 0),
        (1, 4, 0, 256, 256, 4097, 2048, 1), (2, 1, 0, 256, 256, 1025, 512, 0), (2, 1, 1, 256, 256, 1025, 8, 0),
        (2, 2, 0, 320, 256, 1025, 17408, 0), (2, 3, 0, 256, 256, 1025, 10752, 0), (2, 4, 0, 256, 256, 5121, 2048, 1),
        (2, 4, 0, 256, 256, 34816, 4096, 0), (3, 1, 0, 256, 256, 2050, 512, 0), (3, 1, 1, 256, 256, 2050, 264, 0),
        (3, 2, 0, 320, 256, 2050, 17408, 0), (4, 1, 0, 256, 256, 3073, 512, 0), (4, 1, 1, 256, 256, 3073, 1000, 0),
        (4, 2, 0, 320, 256, 3073, 17408, 0),
    ],
    (0, 1, 0, 1): [
        (1, 1, 0, 256, 2, 6, 512, 1), (1, 1, 1, 256, 2, 6, 8, 1), (1, 1, 1, 320, 2, 6, 4352, 1), (1, 1, 1, 384, 2, 5, 5376, 1),
        (1, 1, 1, 448, 2, 7, 6400, 1), (1, 1, 1, 512, 2, 6, 7424, 1), (1, 2, 0, 256, 256, 4097, 1024, 1),
        (1, 3, 0, 256, 256, 4097, 1536, 1), (1, 4, 0, 256, 256, 4097, 2048, 1), (2, 1, 0, 256, 256, 1025, 512, 1),
        (2, 1, 1, 256, 256, 1025, 264, 1), (2, 2, 0, 256, 256, 9217, 1024, 1), (2, 3, 0, 256, 256, 5121, 1536, 1),
        (2, 4, 0, 256, 256, 5121, 2048, 1), (3, 1, 0, 256, 256, 2050, 512, 1), (3, 1, 1, 256, 256, 2050, 1000, 1),
        (4, 1, 0, 256, 256, 3073, 512, 1), (4, 1, 1, 256, 256, 3073, 8, 1), (4, 2, 0, 256, 256, 7169, 1024, 1),
    ],
    (0, 1, 1, 0): [
        (1, 1, 0, 256, 2, 6, 512, 0), (1, 1, 1, 256, 2, 6, 8, 0), (1, 2, 0, 320, 2, 6, 17408, 0), (1, 3, 0, 256, 2, 5, 10752, 0),
        (2, 1, 0, 256, 256, 1025, 512, 0), (2, 1, 1, 256, 256, 1025, 264, 0), (2, 2, 0, 320, 256, 1025, 17408, 0),
        (2, 3, 0, 256, 256, 1025, 10752, 0), (3, 1, 0, 256, 256, 2050, 512, 0), (3, 1, 1, 256, 256, 2050, 1000, 0),
        (3, 2, 0, 320, 256, 2050, 17408, 0), (4, 1, 0, 256, 256, 3073, 512, 0), (4, 1, 1, 256, 256, 3073, 8, 0),
        (4, 2, 0, 320, 256, 3073, 17408, 0),
    ],
    (0, 1, 1, 1): [
        (1, 1, 0, 256, 2, 6, 512, 0), (1, 1, 1, 256, 2, 5, 264, 0), (2, 1, 0, 256, 256, 1025, 512, 0),
        (2, 1, 1, 256, 256, 1025, 1000, 0), (3, 1, 0, 256, 256, 2050, 512, 0), (3, 1, 1, 256, 256, 2050, 8, 0),
        (4, 1, 0, 256, 256, 3073, 512, 0), (4, 1, 1, 256, 256, 3073, 264, 0),
    ],
    (0, 1, 2, 0): [
        (1, 1, 0, 256, 24, 96, 512, 0), (1, 1, 1, 256, 24, 96, 264, 0), (1, 1, 1, 256, 512, 2048, 8, 0),
        (1, 2, 0, 256, 24, 96, 1024, 0), (1, 3, 0, 256, 24, 96, 1536, 0), (1, 4, 0, 256, 24, 96, 2048, 0),
        (2, 1, 0, 256, 256, 1056, 512, 0), (2, 1, 1, 256, 256, 1056, 1000, 0), (2, 2, 0, 256, 256, 1056, 1024, 0),
        (3, 1, 0, 256, 512, 4160, 512, 0), (3, 1, 1, 256, 512, 4160, 8, 0), (4, 1, 0, 256, 512, 8192, 512, 0),
        (4, 1, 1, 256, 512, 8192, 264, 0),
    ],
    (0, 1, 2, 1): [
        (1, 1, 0, 256, 24, 96, 512, 0), (1, 1, 1, 256, 24, 96, 1000, 0), (1, 2, 0, 256, 24, 96, 1024, 0),
        (1, 3, 0, 256, 24, 96, 1536, 0), (1, 4, 0, 256, 24, 96, 2048, 0), (2, 1, 0, 256, 256, 1056, 512, 0),
        (2, 1, 1, 256, 256, 1056, 8, 0), (2, 2, 0, 256, 256, 1056, 1024, 0), (3, 1, 0, 256, 512, 4160, 512, 0),
        (3, 1, 1, 256, 512, 4160, 264, 0), (4, 1, 0, 256, 512, 8192, 512, 0), (4, 1, 1, 256, 512, 8192, 1000, 0),
    ],
    (0, 1, 3, 0): [
        (1, 1, 0, 256, 2, 6, 512, 0), (1, 1, 1, 256, 2, 7, 1000, 0), (1, 2, 0, 256, 2, 7, 1024, 0), (1, 3, 0, 256, 2, 5, 1536, 0),
        (1, 4, 0, 256, 2, 6, 2048, 0), (2, 1, 0, 256, 256, 1025, 512, 0), (2, 1, 1, 256, 256, 1025, 8, 0),
        (2, 2, 0, 256, 256, 1025, 1024, 0), (3, 1, 0, 256, 512, 4097, 512, 0), (3, 1, 1, 256, 512, 4097, 264, 0),
        (4, 1, 0, 256, 512, 6145, 512, 0), (4, 1, 1, 256, 512, 6145, 1000, 0),
    ],
    (0, 1, 3, 1): [
        (1, 1, 0, 256, 2, 6, 512, 0), (1, 1, 1, 256, 2, 6, 8, 0), (1, 2, 0, 256, 2, 7, 1024, 0), (1, 3, 0, 256, 2, 5, 1536, 0),
        (1, 4, 0, 256, 2, 6, 2048, 0), (2, 1, 0, 256, 256, 1025, 512, 0), (2, 1, 1, 256, 256, 1025, 264, 0),
        (2, 2, 0, 256, 256, 1025, 1024, 0), (3, 1, 0, 256, 512, 4097, 512, 0), (3, 1, 1, 256, 512, 4097, 1000, 0),
        (4, 1, 0, 256, 512, 6145, 512, 0), (4, 1, 1, 256, 512, 6145, 8, 0),
    ],
    (1, 0, 0, 0): [
        (1, 4, 0, 128, 1, 1, 512, 1), (1, 4, 0, 384, 8, 30, 1536, 0), (1, 4, 0, 640, 5, 20, 2560, 1), (1, 4, 0, 896, 1, 1, 3584, 0),
        (1, 16, 0, 1024, 240, 3840, 4096, 0), (1, 16, 0, 1024, 241, 3841, 4096, 0), (2, 4, 0, 576, 1, 1, 4608, 1),
        (2, 4, 0, 576, 5, 20, 4608, 1), (2, 4, 0, 832, 8, 30, 6656, 0), (2, 8, 0, 1024, 240, 1920, 8192, 0),
        (2, 8, 0, 1024, 241, 1921, 8192, 0), (4, 4, 0, 576, 1, 1, 9216, 1), (4, 4, 0, 640, 5, 20, 10240, 1),
        (4, 4, 0, 832, 8, 30, 13312, 0),
    ],
    (1, 0, 0, 1): [
        (1, 4, 0, 192, 1, 2, 768, 1), (1, 4, 0, 448, 4, 15, 1792, 1), (1, 4, 0, 704, 6, 24, 2816, 1), (1, 4, 0, 960, 1, 2, 3840, 1),
        (1, 16, 0, 1024, 240, 3840, 4096, 1), (1, 16, 0, 1024, 241, 3846, 4096, 1), (2, 4, 0, 640, 1, 2, 5120, 1),
        (2, 4, 0, 768, 6, 24, 6144, 1), (2, 4, 0, 896, 4, 15, 7168, 1), (2, 8, 0, 1024, 240, 1920, 8192, 1),
        (2, 8, 0, 1024, 241, 1926, 8192, 1), (4, 4, 0, 640, 1, 2, 10240, 1), (4, 4, 0, 704, 6, 24, 11264, 1),
        (4, 4, 0, 896, 4, 15, 14336, 1),
    ],
    (1, 0, 1, 0): [
        (1, 4, 0, 256, 1, 3, 1024, 0), (1, 4, 0, 512, 5, 17, 2048, 0), (1, 4, 0, 768, 7, 28, 3072, 0), (1, 4, 0, 1024, 1, 3, 4096, 0),
        (1, 16, 0, 1024, 240, 3840, 4096, 0), (1, 16, 0, 1024, 241, 3851, 4096, 0), (2, 4, 0, 704, 1, 3, 5632, 0),
        (2, 4, 0, 896, 7, 28, 7168, 0), (2, 4, 0, 960, 5, 17, 7680, 0), (2, 8, 0, 1024, 240, 1920, 8192, 0),
        (2, 8, 0, 1024, 241, 1924, 8192, 0), (4, 4, 0, 704, 1, 3, 11264, 0), (4, 4, 0, 832, 7, 28, 13312, 0),
        (4, 4, 0, 960, 5, 17, 15360, 0),
    ],
    (1, 0, 1, 1): [
        (1, 4, 0, 320, 1, 1, 1280, 0), (1, 4, 0, 576, 6, 22, 2304, 0), (1, 4, 0, 832, 8, 32, 3328, 0),
        (1, 16, 0, 1024, 240, 3840, 4096, 0), (1, 16, 0, 1024, 241, 3841, 4096, 0), (2, 4, 0, 768, 1, 1, 6144, 0),
        (2, 4, 0, 1024, 6, 22, 8192, 0), (2, 4, 0, 1024, 8, 32, 8192, 0), (2, 8, 0, 1024, 240, 1920, 8192, 0),
        (2, 8, 0, 1024, 241, 1922, 8192, 0), (4, 4, 0, 768, 1, 1, 12288, 0), (4, 4, 0, 960, 8, 32, 15360, 0),
        (4, 4, 0, 1024, 6, 22, 16384, 0),
    ],
    (1, 1, 0, 0): [
        (1, 4, 0, 128, 1, 1, 1024, 1), (1, 4, 0, 384, 8, 30, 3072, 0), (1, 4, 0, 640, 5, 20, 5120, 1), (1, 4, 0, 896, 1, 1, 7168, 0),
        (1, 16, 0, 1024, 240, 3840, 8192, 0), (1, 16, 0, 1024, 241, 3841, 8192, 0), (2, 4, 0, 576, 1, 1, 9216, 1),
        (2, 4, 0, 576, 5, 20, 9216, 1), (2, 4, 0, 832, 8, 30, 13312, 0), (2, 8, 0, 1024, 240, 1920, 16384, 0),
        (2, 8, 0, 1024, 241, 1921, 16384, 0), (4, 4, 0, 576, 1, 1, 18432, 1), (4, 4, 0, 640, 5, 20, 20480, 1),
        (4, 4, 0, 832, 8, 30, 26624, 0),
    ],
    (1, 1, 0, 1): [
        (1, 4, 0, 192, 1, 2, 1536, 1), (1, 4, 0, 448, 4, 15, 3584, 1), (1, 4, 0, 704, 6, 24, 5632, 1), (1, 4, 0, 960, 1, 2, 7680, 1),
        (1, 16, 0, 1024, 240, 3840, 8192, 1), (1, 16, 0, 1024, 241, 3846, 8192, 1), (2, 4, 0, 640, 1, 2, 10240, 1),
        (2, 4, 0, 768, 6, 24, 12288, 1), (2, 4, 0, 896, 4, 15, 14336, 1), (2, 8, 0, 1024, 240, 1920, 16384, 1),
        (2, 8, 0, 1024, 241, 1926, 16384, 1), (4, 4, 0, 640, 1, 2, 20480, 1), (4, 4, 0, 704, 6, 24, 22528, 1),
        (4, 4, 0, 896, 4, 15, 28672, 1),
    ],
    (1, 1, 1, 0): [
        (1, 4, 0, 256, 1, 3, 2048, 0), (1, 4, 0, 512, 5, 17, 4096, 0), (1, 4, 0, 768, 7, 28, 6144, 0), (1, 4, 0, 1024, 1, 3, 8192, 0),
        (1, 16, 0, 1024, 240, 3840, 8192, 0), (1, 16, 0, 1024, 241, 3851, 8192, 0), (2, 4, 0, 704, 1, 3, 11264, 0),
        (2, 4, 0, 896, 7, 28, 14336, 0), (2, 4, 0, 960, 5, 17, 15360, 0), (2, 8, 0, 1024, 240, 1920, 16384, 0),
        (2, 8, 0, 1024, 241, 1924, 16384, 0), (4, 4, 0, 704, 1, 3, 22528, 0), (4, 4, 0, 832, 7, 28, 26624, 0),
        (4, 4, 0, 960, 5, 17, 30720, 0),
    ],
    (1, 1, 1, 1): [
        (1, 4, 0, 320, 1, 1, 2560, 0), (1, 4, 0, 576, 6, 22, 4608, 0), (1, 4, 0, 832, 8, 32, 6656, 0),
        (1, 16, 0, 1024, 240, 3840, 8192, 0), (1, 16, 0, 1024, 241, 3841, 8192, 0), (2, 4, 0, 768, 1, 1, 12288, 0),
        (2, 4, 0, 1024, 6, 22, 16384, 0), (2, 4, 0, 1024, 8, 32, 16384, 0), (2, 8, 0, 1024, 240, 1920, 16384, 0),
        (2, 8, 0, 1024, 241, 1922, 16384, 0), (4, 4, 0, 768, 1, 1, 24576, 0), (4, 4, 0, 960, 8, 32, 30720, 0),
        (4, 4, 0, 1024, 6, 22, 32768, 0),
    ],
}

# Classes the sweep of test_gemv_picked.py reaches but no case runs: the smallest swept shape (NU x K, the weight rows are NU, or
# 2 NU for q|k|v and gate|up) has more than CAP_BYTES of weights.  class: (NU, K) of that shape, asserted by the CPU test.
EXCLUDED = {
    (0, F32, PLAIN, 1, 3, 2, 0): (128256, 512),       # 250 MB
    (0, F32, RESIDUAL, 1, 2, 2, 0): (34816, 2560),    # 340 MB
    (0, F32, RESIDUAL, 1, 2, 4, 0): (34816, 2048),    # 272 MB
    (0, F32, RESIDUAL, 1, 3, 2, 0): (128256, 2560),   # 1252 MB
    (0, F32, RESIDUAL, 1, 4, 2, 0): (16384, 5632),    # 352 MB
    (0, F16, PLAIN, 1, 3, 2, 0): (128256, 1024),      # 250 MB
    (0, F16, RESIDUAL, 0, 1, 4, 0): (4097, 32768),    # 256 MB + one row: the first K = 16 * 4 chunks past the split-K cap
    (0, F16, RESIDUAL, 0, 2, 4, 0): (34816, 4096),    # 272 MB
    (0, F16, RESIDUAL, 1, 2, 2, 0): (34816, 5120),    # 340 MB
    (0, F16, RESIDUAL, 1, 2, 3, 0): (34816, 4608),    # 306 MB
    (0, F16, RESIDUAL, 1, 2, 4, 0): (34816, 4096),    # 272 MB
    (0, F16, RESIDUAL, 1, 3, 2, 0): (128256, 5120),   # 1252 MB
}

Case = namedtuple("Case", "kernel wt mode norm a b guard threads grid NU K argmax")
CASES = sorted((Case(*key, *row) for key, rows in TABLE.items() for row in rows), key=lambda c: (c.wt, c.K, c.mode, c.NU, c.norm, c.kernel, c.argmax))


def cls(c):
    return (c.kernel, c.wt, c.mode, c.norm, c.a, c.b, c.guard)


def desc_cls(d):
    """The class of a 16-word descriptor (GemvDesc)."""
    return (d[0], d[1], d[2], d[3], d[6], d[7], d[8])


def case_id(c):
    form = f"sk-ch{c.a}-rw{c.b}" if c.kernel else f"upw{c.a}-u{c.b}" + ("-guard" if c.guard else "")
    return f"{'f16' if c.wt == F16 else 'f32'}-{MODE_NAMES[c.mode]}{'-norm' if c.norm else ''}{'-argmax' if c.argmax else ''}-{form}-NU{c.NU}-K{c.K}"


def rpu(mode):
    return 2 if mode in (QKV, GATEUP) else 1


def weight_bytes(wt, mode, NU, K):
    return NU * rpu(mode) * K * (2 if wt == F16 else 4)


def qkv_shape(c):
    """(H, Hkv, D, kv16, pos) of a q|k|v case: whole heads of 64 or 128, (H + 2 Hkv) D = 2 NU."""
    D = 128 if (c.NU % 64 == 0 and c.NU >= 192 and (c.K // 8) % 2 == 0) else 64
    n = 2 * c.NU // D
    assert n * D == 2 * c.NU and n >= 3, c
    Hkv = 1 if n < 6 else 2
    return n - 2 * Hkv, Hkv, D, (c.K // 8 + c.NU // 32 + c.norm) % 2 == 1, (0, 3)[(c.a + c.guard + c.wt) % 2]


def seg_rows(c):
    """GemvArgs::seg_rows of the case, as the ABI entry passes them."""
    if c.mode == QKV:
        H, Hkv, D, _, _ = qkv_shape(c)
        return H * D, Hkv * D, Hkv * D
    return (c.NU, c.NU, 0) if c.mode == GATEUP else (c.NU, 0, 0)


def load_plan():
    """plan(w_type, mode, rows0, rows1, rows2, K, n_cu, norm, fused_argmax) -> the 16 words launch_gemv would launch with, or None
    where it refuses (nfai_hip_debug_gemv_plan: host arithmetic, no device)."""
    import ctypes as C
    from nfai_amd import _lib
    lib = _lib.load()
    f = lib.nfai_hip_debug_gemv_plan
    f.argtypes = [C.c_int32, C.c_int32] + [C.c_uint32] * 5 + [C.c_int32, C.c_int32, C.POINTER(C.c_uint32)]
    f.restype = C.c_int32
    buf = (C.c_uint32 * 16)()

    def plan(*args):
        return None if f(*args, buf) else tuple(buf)
    return plan


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
MAX_ROWS = {}
for _c in CASES:
    MAX_ROWS[(_c.wt, _c.K)] = max(MAX_ROWS.get((_c.wt, _c.K), 0), _c.NU * rpu(_c.mode))


@functools.lru_cache(maxsize=2)
def weights(wt, K):
    """Every weight row any case of (w_type, K) uses, 0.02 N(0, 1) in the weight type; a case takes the first rows.  Above 4 M
    elements the normal draws are a block of 1021 rows (a prime period) repeated, with the first 8 columns of every row drawn
    afresh, so rows stay distinct."""
    rows = MAX_ROWS[(wt, K)]
    r = np.random.Generator(np.random.PCG64(77 + 2 * K + wt))
    dt = np.float16 if wt == F16 else np.float32
    if rows * K <= 1 << 22:
        return (0.02 * r.standard_normal((rows, K), dtype=np.float32)).astype(dt)
    base = (0.02 * r.standard_normal((1021, K), dtype=np.float32)).astype(dt)
    W = np.tile(base, ((rows + 1020) // 1021, 1))[:rows]
    W[:, :8] = (0.02 * r.standard_normal((rows, 8), dtype=np.float32)).astype(dt)
    return W


def inputs(c):
    """W [rows][K] (q | k | v or gate | up rows one after the other), x ~ N(0, 1), gamma = 1 + 0.1 N(0, 1), residual ~ N(0, 1)."""
    r = np.random.Generator(np.random.PCG64(1000003 * c.K + 7919 * c.NU + 101 * c.mode + 13 * c.norm + 5 * c.wt + c.argmax + 31 * c.kernel))
    W = weights(c.wt, c.K)[:c.NU * rpu(c.mode)]
    x = r.standard_normal(c.K).astype(np.float32)
    g = (1 + 0.1 * r.standard_normal(c.K)).astype(np.float32)
    res = r.standard_normal(c.NU).astype(np.float32)
    return W, x, g, res


# ---- float64 reference and bars ---------------------------------------------------------------------------------------------------
def _ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def _gemv64(W, xv, tile=4096):
    """W @ xv in float64 on the stored operands, and gemv_tol (tests/test_gpu_ops.py) of every row, a tile of rows at a time."""
    from test_gpu_ops import gemv_tol
    s, tol = np.empty(W.shape[0]), np.empty(W.shape[0])
    for r0 in range(0, W.shape[0], tile):
        Wt = W[r0:r0 + tile].astype(np.float64)
        s[r0:r0 + tile] = Wt @ xv
        tol[r0:r0 + tile] = gemv_tol(Wt, xv)
    return s, tol


def reference(c, W, x, g, res):
    """(want, bar) of the case in float64, RMSNorm, rotation, SiLU * up and the residual included.  q|k|v: want and bar cover the
    rows q | k | v as the launch orders them (the cache rows' fp16 allowance is the caller's); the rotation angle is pos * freq
    with the fp32 frequencies the launch is given."""
    x64 = x.astype(np.float64)
    xv = x64 / np.sqrt(np.mean(x64 * x64) + EPS) * g.astype(np.float64) if c.norm else x64
    s, tol = _gemv64(W, xv)
    if c.mode == PLAIN:
        return s, tol
    if c.mode == RESIDUAL:
        want = res.astype(np.float64) + s
        return want, tol + _ulp32(want)
    if c.mode == GATEUP:
        gate, up, tg, tu = s[:c.NU], s[c.NU:], tol[:c.NU], tol[c.NU:]
        silu = gate / (1.0 + np.exp(-gate))
        want = up * silu
        return want, np.abs(silu) * tu + 1.1 * np.abs(up) * tg + _ulp32(want)
    H, Hkv, D, _, pos = qkv_shape(c)
    want, bar = s.copy(), tol.copy()
    nrot = (H + Hkv) * D                                   # q and k rows rotate in pairs (2i, 2i + 1); v rows are stored as they are
    th = rope_freqs(D).astype(np.float64) * pos
    cs, sn = np.tile(np.cos(th), H + Hkv), np.tile(np.sin(th), H + Hkv)
    a, b = s[0:nrot:2], s[1:nrot:2]
    want[0:nrot:2] = cs * a - sn * b
    want[1:nrot:2] = sn * a + cs * b
    pair = tol[0:nrot:2] + tol[1:nrot:2] + 2e-6 * pos / 8  # + the device's cos / sin at pos, as test_gemv_qkv_rope_kvwrite allows it
    bar[0:nrot:2] = pair
    bar[1:nrot:2] = pair
    return want, bar


def rope_freqs(D):
    from oracle import np_oracle as npo
    return npo.rope_freqs(D, 500000.0).astype(np.float32)


def argmax_gap(want, bar):
    """(first index of the largest reference output, its margin over the runner-up, the larger of the two rows' bars)."""
    i = int(np.argmax(want))
    rest = np.delete(want, i)
    if rest.size == 0:
        return i, np.inf, float(bar[i])
    j = int(np.argmax(rest))
    j += j >= i
    return i, float(want[i] - want[j]), float(max(bar[i], bar[j]))
