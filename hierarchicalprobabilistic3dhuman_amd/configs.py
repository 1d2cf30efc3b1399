"""Configuration values the hot path reads.

The reference keeps these in a yacs ``CfgNode`` (configs/poseMF_shapeGaussian_net_config.py:4-24);
the hot path only ever reads attributes, so any attribute bag with the same names works.  yacs
objects are accepted unchanged wherever a ``config`` is taken.
"""
from types import SimpleNamespace

# SMPL kinematic tree (public constant; the reference reads it from the SMPL pkl at run_predict.py:65).
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]

NUM_VERTS = 6890
NUM_JOINTS = 24

# smplx VertexJointSelector: 21 vertices appended after the 24 kinematic joints
# (face, feet, left-hand tips, right-hand tips) -- SURVEY.md section 8(a) note.
SMPLX_EXTRA_VERTEX_IDS = [332, 6260, 2800, 4071, 583,
                          3216, 3226, 3387, 6617, 6624, 6787,
                          2746, 2319, 2445, 2556, 2673,
                          6191, 5782, 5905, 6016, 6133]


def _loss_stage(overreg, pose, shape, joints2d, glob_rotmats, verts3d, joints3d, j2d_loss_on):
    return SimpleNamespace(REDUCTION="mean", MF_OVERREG=overreg, J2D_LOSS_ON=j2d_loss_on,
                           WEIGHTS=SimpleNamespace(POSE=pose, SHAPE=shape, JOINTS2D=joints2d, GLOB_ROTMATS=glob_rotmats,
                                                   VERTS3D=verts3d, JOINTS3D=joints3d))


def _synth_data():
    """configs/poseMF_shapeGaussian_net_config.py:36-80: the values the synthetic-data front end reads (train_augmentation) -- camera,
    box, proxy-representation and RGB augmentation; probabilities, ranges and class lists only."""
    proxy_rep = SimpleNamespace(
        REMOVE_PARTS_CLASSES=list(range(1, 25)),                                     # DensePose part classes
        REMOVE_PARTS_PROBS=[0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.1, 0.1,
                            0.1, 0.1, 0.05, 0.05, 0.05, 0.05, 0.1, 0.1, 0.1, 0.1, 0.05, 0.05],
        REMOVE_APPENDAGE_JOINTS_PROB=0.5, REMOVE_JOINTS_INDICES=[7, 8, 9, 10, 13, 14, 15, 16], REMOVE_JOINTS_PROB=0.1,
        DELTA_J2D_DEV_RANGE=[-6, 6], JOINTS_TO_SWAP=[[5, 6], [11, 12]], JOINTS_SWAP_PROB=0.1, OCCLUDE_BOX_DIM=48,
        OCCLUDE_BOX_PROB=0.1, OCCLUDE_BOTTOM_PROB=0.02, OCCLUDE_TOP_PROB=0.005, OCCLUDE_VERTICAL_PROB=0.05, EXTREME_CROP_PROB=0.1)
    rgb = SimpleNamespace(OCCLUDE_BOTTOM_PROB=0.02, OCCLUDE_TOP_PROB=0.005, OCCLUDE_VERTICAL_PROB=0.05, PIXEL_CHANNEL_NOISE=0.2,
                          LIGHT_LOC_RANGE=[0.05, 3.0], LIGHT_AMBIENT_RANGE=[0.4, 0.8], LIGHT_DIFFUSE_RANGE=[0.4, 0.8],
                          LIGHT_SPECULAR_RANGE=[0.0, 0.5])                           # :73-76, textured_renderer.augment_light
    bbox = SimpleNamespace(DELTA_SCALE_RANGE=[-0.3, 0.2], DELTA_CENTRE_RANGE=[-5, 5])
    return SimpleNamespace(FOCAL_LENGTH=300.0, MEAN_CAM_T=[0.0, -0.2, 2.5],
                           AUGMENT=SimpleNamespace(BBOX=bbox, PROXY_REP=proxy_rep, RGB=rgb,
                                                   SMPL=SimpleNamespace(SHAPE_STD=1.25),                          # :45
                                                   CAM=SimpleNamespace(XY_STD=0.05, DELTA_Z_RANGE=[-0.5, 0.5])))  # :48-49


class _Bag(dict):
    """A dict whose keys are also attributes, like a yacs CfgNode: models/pose2D_hrnet.py indexes its config (cfg['MODEL']['EXTRA']),
    predict/predict_hrnet.py reads attributes (hrnet_config.MODEL.IMAGE_SIZE)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)

    def __setattr__(self, name, value):
        self[name] = value

    def __deepcopy__(self, memo):
        import copy
        return _Bag((k, copy.deepcopy(v, memo)) for k, v in self.items())


def get_pose2D_hrnet_cfg_defaults():
    """The values of configs/pose2D_hrnet_config.py:17-55 (HRNet-W48 at 384 x 288), as an attribute / index bag; a fresh object per call."""
    def stage(modules, branches, blocks, channels):
        return _Bag(NUM_MODULES=modules, NUM_BRANCHES=branches, BLOCK="BASIC", NUM_BLOCKS=list(blocks), NUM_CHANNELS=list(channels),
                    FUSE_METHOD="SUM")
    extra = _Bag(PRETRAINED_LAYERS=["conv1", "bn1", "conv2", "bn2", "layer1", "transition1", "stage2", "transition2", "stage3",
                                    "transition3", "stage4"],
                 FINAL_CONV_KERNEL=1,
                 STAGE2=stage(1, 2, [4, 4], [48, 96]),
                 STAGE3=stage(4, 3, [4, 4, 4], [48, 96, 192]),
                 STAGE4=stage(3, 4, [4, 4, 4, 4], [48, 96, 192, 384]))
    return _Bag(MODEL=_Bag(NUM_JOINTS=17, IMAGE_SIZE=[288, 384], HEATMAP_SIZE=[72, 96], EXTRA=extra),     # width, height
                TEST=_Bag(POST_PROCESS=False, OBJECT_DET_THRESH=0.95))


def get_cfg_defaults():
    """Values of configs/poseMF_shapeGaussian_net_config.py:8-24 that the inference path reads, of :83-110 that
    matrix_fisher_loss.PoseMFShapeGaussianLoss reads (LOSS.STAGE1 / STAGE2: REDUCTION, MF_OVERREG, WEIGHTS), and of :29, :36-80 that
    the synthetic-data training front end reads (TRAIN.BATCH_SIZE, TRAIN.SYNTH_DATA), and of :28-33, :84-86, :91, :103 that the
    training loop reads (TRAIN.NUM_EPOCHS ... NUM_WORKERS, LOSS.SAMPLE_ON_CPU / NUM_SAMPLES / STAGE_CHANGE_EPOCH, J2D_LOSS_ON)."""
    return SimpleNamespace(
        MODEL=SimpleNamespace(NUM_IN_CHANNELS=18, NUM_RESNET_LAYERS=18, EMBED_DIM=256,
                              DELTA_I=True, DELTA_I_WEIGHT=1.0, NUM_SMPL_BETAS=10),
        DATA=SimpleNamespace(PROXY_REP_SIZE=256, HEATMAP_GAUSSIAN_STD=4.0, EDGE_NMS=True,
                             EDGE_THRESHOLD=0.0, EDGE_GAUSSIAN_STD=1.0, EDGE_GAUSSIAN_SIZE=5,
                             BBOX_THRESHOLD=0.95, BBOX_SCALE_FACTOR=1.2),
        LOSS=SimpleNamespace(SAMPLE_ON_CPU=True, NUM_SAMPLES=8, STAGE_CHANGE_EPOCH=66,
                             STAGE1=_loss_stage(1.005, 80.0, 50.0, 5000.0, 5000.0, 0.0, 0.0, "means"),
                             STAGE2=_loss_stage(1.005, 10.0, 80.0, 30000.0, 5000.0, 5000.0, 5000.0, "means+samples")),
        TRAIN=SimpleNamespace(NUM_EPOCHS=300, BATCH_SIZE=72, LR=0.0001, EPOCHS_PER_SAVE=5, PIN_MEMORY=True, NUM_WORKERS=2,
                              SYNTH_DATA=_synth_data()),
    )
