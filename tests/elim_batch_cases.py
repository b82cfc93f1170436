"""Data only: the shapes (m, ncols, batch) that tests/test_gpu_elim_batch.py runs as random stacks, and the sizes of its inverse test.
tests/test_elim_batch_plan.py checks that together they reach every kernel variant gf2_elim_batch_plan can choose."""

SHAPES = [
    (1, 1, 256), (1, 64, 130), (7, 5, 1000), (10, 10, 4096), (33, 100, 300), (64, 64, 1024), (64, 65, 257),
    (63, 1024, 64), (64, 1024, 70), (65, 64, 200), (65, 130, 129), (100, 100, 256), (128, 256, 64),
    (200, 300, 40), (256, 256, 40), (300, 1000, 7), (511, 65, 10), (512, 512, 9), (512, 1024, 5),
    # rows of 3-4 and 5-8 words in a wave (the list above has 1, 2 and 16)
    (40, 193, 100), (64, 512, 66), (17, 321, 90),
]

# (n, matrices) of the inverse test
INVERSE_SIZES = [(1, 256), (10, 256), (64, 256), (65, 256), (100, 256), (256, 24), (512, 24)]
