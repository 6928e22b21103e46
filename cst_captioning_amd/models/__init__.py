from .caption_model import CaptionModel
from .criteria import CrossEntropyCriterion, RewardCriterion, GroupCriterion, reward_mask
from .modules import FeatPool, FeatExpander, RNNUnit, MANet, TemporalAttention

__all__ = ['CaptionModel', 'CrossEntropyCriterion', 'RewardCriterion', 'GroupCriterion',
           'reward_mask', 'FeatPool', 'FeatExpander', 'RNNUnit', 'MANet', 'TemporalAttention']
