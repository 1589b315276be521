"""Import-path shim: ``from spec.utils.renderer_cam import render_image_group`` (spec/tester.py:33, spec/trainer.py:41 of the
reference) resolves to this build's device rasteriser (spec_amd/render.py): the reference's geometry and file names, its own
declared shading - not pyrender's look.  ``render_image_group`` takes the reference's full argument list (``alpha`` is accepted
and ignored, ``keypoints_2d`` is drawn on the device by this project's own drawing contract).  ``RendererCam`` (the training-time TensorBoard grid) is not provided."""
import numpy as np

from spec_amd.render import render_image_group  # noqa: F401


def render_overlay_image(image, camera_translation, vertices, camera_rotation, focal_length, camera_center, mesh_color='gray',
                         alpha=1.0, faces=None, sideview_angle=0, mesh_filename=None, add_ground_plane=True):
    """The reference's call (renderer_cam.py:44-57): ``image`` (H, W, 3) floats in [0, 1] -> floats in [0, 1].  ``alpha`` other
    than 1 and side-view angles other than 0 / 270 are refused; ``camera_translation`` is NOT flipped in place as the reference
    does to its caller's array."""
    import torch
    from spec_amd import render
    if alpha != 1.0 or sideview_angle not in (0, 270):
        raise NotImplementedError('the device rasteriser draws opaque meshes at side-view angles 0 and 270')
    frame = torch.from_numpy(np.clip(np.asarray(image, np.float64) * 255.0, 0, 255).astype(np.uint8)).to('cuda')
    side = sideview_angle == 270
    out = render.render_overlay(frame, np.asarray(vertices, np.float32), np.asarray(camera_translation, np.float32),
                                np.asarray(camera_rotation, np.float32), focal_length, camera_center, faces=faces, color=mesh_color,
                                side_view=side, ground_plane=side and add_ground_plane)
    if mesh_filename:
        table = render.device_faces(faces, out.device).cpu().numpy()
        render.write_obj(mesh_filename, np.asarray(vertices, np.float32) * np.array([1., -1., -1.], np.float32), table)
    return out.cpu().numpy().astype(np.float32) / 255.0
