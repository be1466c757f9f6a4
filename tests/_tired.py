"""Names of the fixtures at the driver-monitoring YAMLs' spatial strides (tests/golden/make_golden_tired.py): the
grayscale cases of tests/_gray.py with RESNET.SPATIAL_STRIDES [[1,1],[1,1],[2,2],[2,2]], head extent 1 x 3 x 3 at crop
64.  Models and clips come from _gray.build_gray / _gray.gray_inputs, which load any fixture by name."""
TIRED_CASES = ["fast_r18_gray_tired_s64", "dual_r18_gray_tired_s64"]
EXTENT = 9          # To * Ho * Wo of the pooled head features
TRAIN_LOGITS = 27   # EXTENT * MODEL.NUM_CLASSES
