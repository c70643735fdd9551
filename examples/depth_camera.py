"""The reference's camera example (examples/aliengo_with_camera.py), batched: RGB, depth and segmentation images of every env from the
``robotcam`` camera on aliengo's trunk, saved as .npy instead of shown with cv2; and a tracking video frame of every env
(``env.render('rgb_array')``) at the end, and one with two ghosts (20 steps behind and ahead) and the velocity arrows.

    python examples/depth_camera.py [scene] [num_envs] [steps]"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from gym_quadruped_amd.quadruped_env import QuadrupedEnv  # noqa: E402
from gym_quadruped_amd.sensors import Camera  # noqa: E402
from gym_quadruped_amd.utils.visual import velocity_markers  # noqa: E402

robot_name = 'aliengo'
scene_name = sys.argv[1] if len(sys.argv) > 1 else 'stairs'   # "flat", "stairs", "perlin", "random_boxes", ...
num_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 16
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100

env = QuadrupedEnv(
    robot=robot_name,
    scene=scene_name,
    ref_base_lin_vel=0.5,
    base_vel_command_type='forward',
    state_obs_names=tuple(QuadrupedEnv.ALL_OBS),
    num_envs=num_envs,
)
obs = env.reset()

cam = Camera(
    width=640,
    height=480,
    fps=30,
    mj_model=env.robot_model,
    mj_data=env.sim_data,
    cam_name='robotcam',  # camera must be inserted on the .xml file of the robot in order to work
    save_dir='data_',
    rgb=True,             # cam.image: [N, H, W, 3] uint8 (default Appearance: the model's geom colours, a checker floor)
)

for _ in range(steps):
    sim_time = float(env.simulation_time[0])            # every env advances in lock step
    action = env.action_space.sample() * 0
    state, reward, is_terminated, is_truncated, info = env.step(action=action)
    if sim_time - cam.last_sim_time >= cam.interval:    # camera at its own fps
        cam.shoot(autosave=True, img=True)              # image [N, H, W, 3], depth [N, H, W] and seg [N, H, W] as .npy
        cam.last_sim_time = float(env.simulation_time[0])
frame = env.render('rgb_array')                         # [N, 240, 320, 3] uint8 from a camera tracking each base
Path(cam.save_dir).mkdir(parents=True, exist_ok=True)
np.save(Path(cam.save_dir) / 'render.npy', frame.cpu().numpy())

# ghosts: the pose 20 steps behind and 20 steps ahead of the current one, drawn translucent next to it, with the reference render()'s
# velocity arrows (commanded: orange, actual: cyan)
behind = env.qpos.clone()
for _ in range(20):
    env.step(action=env.action_space.sample() * 0)
now = env.state_dict()
for _ in range(20):
    env.step(action=env.action_space.sample() * 0)
ahead = env.qpos.clone()
env.load_state_dict(now)                                # back to the middle pose
ghosts = torch.stack([behind, ahead], 1)                # [N, 2, 19]
frame = env.render('rgb_array', True, ghosts, 0.35, markers=velocity_markers(env))   # tinted robot, two ghosts, two arrows
np.save(Path(cam.save_dir) / 'render_ghosts.npy', frame.cpu().numpy())
env.close()
