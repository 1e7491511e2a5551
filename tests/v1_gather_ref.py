"""Host references shared by the tests of the v1 tubelet gathers: the im2col of a clip and the uint8 normalise."""
import torch

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalise_u8(frames):
    """uint8 [..., 3] (channel last) -> fp32 of the same shape: ClipToTensor (/ 255) and Normalize ((v - mean) / std), in fp32 and
    in this order"""
    return (frames.float() / 255 - torch.tensor(MEAN)) / torch.tensor(STD)


def im2col_ref(video, keep, tb, p):
    """video fp32 [B, T, 3, img, img], keep int64 [B, tubes, n] -> [B * tubes * n, 3 * tb * p * p] in (c, t, py, px) order"""
    B, T, _, img, _ = video.shape
    tubes, g = T // tb, img // p
    x = video.reshape(B, tubes, tb, 3, g, p, g, p).permute(0, 1, 4, 6, 3, 2, 5, 7).reshape(B, tubes, g * g, -1)
    return torch.gather(x, 2, keep[..., None].expand(-1, -1, -1, x.shape[-1])).reshape(B * tubes * keep.shape[2], -1)
