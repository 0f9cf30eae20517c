"""Run a trained checkpoint over the HIP env, headless (reference humanoid/scripts/play.py without its plotting and
joystick, its camera as --render: DESIGN.md §9).

    python -m ti5_isaacgym_amd.scripts.play --checkpoint PATH [--num_envs 9] [--steps 2000] [--mesh_type plane]
        [--command VX VY YAW] [--state_dtype fp32|fp16] [--robot_index 0] [--out DIR]
        [--render DIR [--render_every 2] [--render_size 640 360] [--render_follow 3.0 0.0 1.0]
                      [--render_scene own|all] [--render_terrain_shadow] [--render_urdf PATH]]
        [--depth DIR [--depth_size 64 48] [--depth_every 2] [--depth_mount X Y Z ROLL PITCH YAW]
                     [--depth_range 0.1 3.0] [--depth_noise] [--depth_latency LO HI]]

The reference play's config changes (episode_length_s 1000, the noise curriculum off), its loop -- the deterministic
policy (DHOnPolicyRunner.get_inference_policy(graphed=True): the first conv and the actor kernel as one replayed HIP
graph per observation buffer), the commands held by writing env.commands before every step -- and its logs:

  DIR/states.npz    one row per step for --robot_index: base_height, foot_z_l/r, foot_forcez_l/r, base_vel_x/y/z,
                    base_vel_yaw, command_x/y/yaw (env.commands as the step read them), and per joint (steps, 12)
                    dof_pos_target (action * action_scale), dof_pos, dof_vel, dof_torque
  DIR/summary.json  the mean per-term episode rewards over the episodes completed during the run (extras["episode"]
                    weighted by the envs that reset that step) and their count; also printed

With --render DIR a camera follows --robot_index (utils/render.py: the robot's collision-level geometry, its shadow
and the terrain).  --render_scene all draws every env's robot and its shadow, as the reference's camera films all of
them (own, the default: only the followed one); --render_terrain_shadow lets a height field cast shadows too.
--render_urdf PATH draws the visual meshes of that robot description (utils/render.RobotMesh.from_urdf; the mesh files
it names must lie where it says) instead of the collision-level primitives; it composes with the two switches, and
summary.json then also counts the last frame's "robot_pixels".  The repository ships no meshes: pass your copy of the
robot description.  Every --render_every-th step is rendered into one preallocated
device buffer and written as DIR/frame_%06d.png after the loop; summary.json then also counts the "frames".  Nothing
here encodes video: e.g. ffmpeg -framerate 50 -i DIR/frame_%06d.png -pix_fmt yuv420p play.mp4.

With --depth DIR a depth camera sensor is bolted to every env's base (utils/render.DepthSensor: one launch draws all
envs) at --depth_mount, the position and roll, pitch, yaw of the camera in the base's frame (it looks along its +x; a
positive pitch looks down; the default is a placeholder, the repository knows no camera of the real robot).  After every
--depth_every-th step the image of --robot_index is kept in a preallocated device buffer; after the loop they are
written as DIR/depth.npy ((frames, H, W) float16, planar depth in metres, --depth_range's FAR where nothing is in
range) and as grey DIR/depth_%06d.png (near white, far black); summary.json then also counts the "depth_frames".
--depth_noise puts the sensor model behind it (utils/render.DepthNoise with DEPTH_NOISE below: depth-squared noise,
dropouts and occlusion shadows, a pixel without a measurement reading FAR) and --depth_latency LO HI serves every env's
image a number of depth frames late, drawn once per env in [LO, HI]; the images written are then the measured ones.

Every logged value stays in device buffers until the run ends: no host read per step.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

SCALARS = ("base_height", "foot_z_l", "foot_z_r", "foot_forcez_l", "foot_forcez_r", "base_vel_x", "command_x",
           "base_vel_y", "command_y", "base_vel_z", "base_vel_yaw", "command_yaw")
PER_JOINT = ("dof_pos_target", "dof_pos", "dof_vel", "dof_torque")
STATE_KEYS = SCALARS + PER_JOINT


def parse(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--checkpoint", required=True)
    p.add_argument("--num_envs", type=int, default=9)
    p.add_argument("--steps", type=int, default=2000)
    p.add_argument("--mesh_type", default="plane")
    p.add_argument("--command", type=float, nargs=3, default=[0.5, 0.0, 0.0], metavar=("VX", "VY", "YAW"))
    p.add_argument("--state_dtype", choices=["fp32", "fp16"], default="fp32")
    p.add_argument("--robot_index", type=int, default=0)
    p.add_argument("--out", default="play_out")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--seed", type=int, default=123145)
    p.add_argument("--render", default=None, metavar="DIR")
    p.add_argument("--render_every", type=int, default=2, metavar="K")
    p.add_argument("--render_size", type=int, nargs=2, default=[640, 360], metavar=("W", "H"))
    p.add_argument("--render_follow", type=float, nargs=3, default=[3.0, 0.0, 1.0], metavar=("X", "Y", "Z"))
    p.add_argument("--render_scene", choices=["own", "all"], default="own")
    p.add_argument("--render_terrain_shadow", action="store_true")
    p.add_argument("--render_urdf", default=None, metavar="PATH")
    p.add_argument("--depth", default=None, metavar="DIR")
    p.add_argument("--depth_size", type=int, nargs=2, default=[64, 48], metavar=("W", "H"))
    p.add_argument("--depth_every", type=int, default=2, metavar="K")
    p.add_argument("--depth_mount", type=float, nargs=6, default=[0.1, 0.0, 0.1, 0.0, 0.6, 0.0],
                   metavar=("X", "Y", "Z", "ROLL", "PITCH", "YAW"))
    p.add_argument("--depth_range", type=float, nargs=2, default=[0.1, 3.0], metavar=("NEAR", "FAR"))
    p.add_argument("--depth_noise", action="store_true")
    p.add_argument("--depth_latency", type=int, nargs=2, default=[0, 0], metavar=("LO", "HI"))
    a = p.parse_args(argv)
    check_render_args(a)
    check_depth_args(a)
    return a


MAX_FRAME_BYTES = 8 << 30
# --depth_noise: a stereo camera's order of magnitude (2 mm + 5 mm/m^2: 4.7 cm at 3 m; 1 % dropouts; every second pixel
# of an occlusion shadow lost) -- a placeholder like the mount, to be replaced by the real sensor's figures
DEPTH_NOISE = dict(sigma0=0.002, sigma2=0.005, p_drop=0.01, p_edge=0.5)
MAX_DEPTH_LATENCY = 15


def num_frames(steps, every):
    """the frames of a run: one after every `every`-th step"""
    return steps // every


def check_render_args(a):
    """Refuse a --render run whose frame buffer (frames x width x height x 4 bytes) would exceed 8 GiB, before any
    device work; --render_urdf without --render, or naming a file that does not exist, likewise."""
    if a.render_urdf is not None:
        if a.render is None:
            raise ValueError("--render_urdf needs --render DIR")
        if not os.path.isfile(a.render_urdf):
            raise FileNotFoundError(f"--render_urdf {a.render_urdf}: no such file")
    if a.render is None:
        return
    w, h = a.render_size
    if a.render_every < 1 or w < 1 or h < 1:
        raise ValueError(f"--render_every {a.render_every} and --render_size {w} {h} must be >= 1")
    frames = num_frames(a.steps, a.render_every)
    if frames * w * h * 4 > MAX_FRAME_BYTES:
        raise ValueError(f"--render: {frames} frames of {w} x {h} pixels need {frames * w * h * 4 / 2 ** 30:.1f} GiB of "
                         "device memory, more than the 8 GiB frame buffer; raise --render_every, lower --steps or "
                         "--render_size")


def check_depth_args(a):
    """Refuse a --depth run with --depth_every or a size below 1, a range that is not 0 < NEAR < FAR <= 200, or a frame
    buffer (frames x width x height x 2 bytes) over 8 GiB, before any device work; --depth_noise or --depth_latency
    without --depth, and a latency that is not 0 <= LO <= HI <= 15, likewise."""
    lo, hi = a.depth_latency
    if a.depth is None:
        if a.depth_noise or (lo, hi) != (0, 0):
            raise ValueError("--depth_noise and --depth_latency need --depth DIR")
        return
    if not 0 <= lo <= hi <= MAX_DEPTH_LATENCY:
        raise ValueError(f"--depth_latency {lo} {hi}: need 0 <= LO <= HI <= {MAX_DEPTH_LATENCY}")
    w, h = a.depth_size
    if a.depth_every < 1 or w < 1 or h < 1:
        raise ValueError(f"--depth_every {a.depth_every} and --depth_size {w} {h} must be >= 1")
    near, far = a.depth_range
    if not 0.0 < near < far <= 200.0:
        raise ValueError(f"--depth_range {near} {far}: need 0 < NEAR < FAR <= 200")
    frames = num_frames(a.steps, a.depth_every)
    if frames * w * h * 2 > MAX_FRAME_BYTES:
        raise ValueError(f"--depth: {frames} frames of {w} x {h} pixels need {frames * w * h * 2 / 2 ** 30:.1f} GiB of "
                         "device memory, more than the 8 GiB frame buffer; raise --depth_every, lower --steps or "
                         "--depth_size")


def main(argv=None):
    from ti5_isaacgym_amd import DHOnPolicyRunner, make_t1_env, task_registry
    from ti5_isaacgym_amd.utils.helpers import class_to_dict
    a = parse(argv)
    if not 0 <= a.robot_index < a.num_envs:
        raise ValueError(f"--robot_index {a.robot_index} is not one of the {a.num_envs} envs")

    def hook(cfg):
        cfg.env.episode_length_s = 1000
        cfg.env.state_dtype = a.state_dtype
        cfg.noise.curriculum = False
        cfg.commands.heading_command = False

    env = make_t1_env(num_envs=a.num_envs, mesh_type=a.mesh_type, seed=a.seed, device=a.device, cfg_hook=hook)
    _, train_cfg = task_registry.get_cfgs("t1_dh_stand")
    runner = DHOnPolicyRunner(env, class_to_dict(train_cfg), None, device=a.device)
    runner.load(a.checkpoint, load_optimizer=False)
    policy = runner.get_inference_policy(device=env.device, graphed=True)

    dev, r, T = env.device, a.robot_index, a.steps
    nj = env.num_actions
    foot_l, foot_r = int(env.feet_indices[0]), int(env.feet_indices[1])
    held = torch.tensor([*a.command, 0.0], device=dev)
    scale = float(env.cfg.control.action_scale)
    scalars = torch.zeros(T, len(SCALARS), device=dev)
    joints = torch.zeros(T, len(PER_JOINT), nj, device=dev)
    ep_keys, ep_sum = None, None
    episodes = torch.zeros((), device=dev)
    renderer = frames = None
    if a.render is not None:
        from ti5_isaacgym_amd.utils.render import Camera, Renderer, RobotMesh, write_png
        w, h = a.render_size
        mesh = RobotMesh.from_urdf(a.render_urdf) if a.render_urdf is not None else None
        renderer = Renderer(env, w, h, [Camera.follow(r, offset=tuple(a.render_follow))],
                            others=a.render_scene == "all", terrain_shadow=a.render_terrain_shadow, mesh=mesh)
        frames = torch.zeros(num_frames(T, a.render_every), 1, h, w, 4, dtype=torch.uint8, device=dev)
    sensor = depth_frames = None
    if a.depth is not None:
        from ti5_isaacgym_amd.utils.render import DepthNoise, DepthSensor, write_png
        dw, dh = a.depth_size
        sensor = DepthSensor(env, dw, dh, a.depth_mount[:3], rpy=a.depth_mount[3:], near=a.depth_range[0],
                             far=a.depth_range[1], dtype=torch.float16,
                             noise=DepthNoise(**DEPTH_NOISE) if a.depth_noise else None,
                             latency=tuple(a.depth_latency), seed=a.seed)
        depth_fresh = torch.zeros(a.num_envs, dtype=torch.uint8, device=dev)   # the envs reset since the last image
        depth_frames = torch.zeros(num_frames(T, a.depth_every), dh, dw, dtype=torch.float16, device=dev)
    obs = env.get_observations()
    with torch.inference_mode():
        for i in range(T):
            actions = policy(obs)
            env.commands[:] = held
            cmd = env.commands[r].clone()   # what this step reads
            obs, _, _, dones, infos = env.step(actions)
            scalars[i] = torch.stack((
                env.root_states[r, 2], env.rigid_state[r, foot_l, 2], env.rigid_state[r, foot_r, 2],
                env.contact_forces[r, foot_l, 2], env.contact_forces[r, foot_r, 2], env.base_lin_vel[r, 0], cmd[0],
                env.base_lin_vel[r, 1], cmd[1], env.base_lin_vel[r, 2], env.base_ang_vel[r, 2], cmd[2]))
            joints[i] = torch.stack((actions[r] * scale, env.dof_pos[r], env.dof_vel[r], env.torques[r]))
            if renderer is not None and (i + 1) % a.render_every == 0:
                renderer.render(frames[(i + 1) // a.render_every - 1])
            if sensor is not None:
                if (i + 1) % a.depth_every == 0:
                    depth_frames[(i + 1) // a.depth_every - 1].copy_(sensor.render(fresh=depth_fresh)[r])
                    depth_fresh.zero_()
                depth_fresh.bitwise_or_(dones.view(torch.uint8))   # seen from where it fell now, fresh at the next image
            ep = infos.get("episode") or {}
            if ep_keys is None:
                ep_keys = [k for k, v in ep.items() if isinstance(v, torch.Tensor)]
                ep_sum = torch.zeros(len(ep_keys), device=dev)
            if ep_keys:   # the step's means over the envs it reset, weighted by their number
                n = (dones > 0).sum().float()
                vals = torch.stack([ep[k].float().reshape(()) for k in ep_keys])
                ep_sum += torch.where(n > 0, vals * n, torch.zeros_like(vals))
                episodes += n
    # the one host read
    scalars, joints = scalars.cpu().numpy(), joints.cpu().numpy()
    count = int(episodes.item())
    sums = ep_sum.cpu().tolist() if ep_keys else []
    os.makedirs(a.out, exist_ok=True)
    states = {k: scalars[:, j] for j, k in enumerate(SCALARS)}
    states.update({k: joints[:, j] for j, k in enumerate(PER_JOINT)})
    np.savez(os.path.join(a.out, "states.npz"), **states)
    summary = {"checkpoint": a.checkpoint, "num_envs": a.num_envs, "steps": T, "command": list(a.command),
               "state_dtype": a.state_dtype, "episodes": count,
               "mean_episode": {k: (s / count if count else None) for k, s in zip(ep_keys or [], sums)}}
    if renderer is not None:
        os.makedirs(a.render, exist_ok=True)
        images = frames.cpu().numpy()
        for k in range(images.shape[0]):
            write_png(os.path.join(a.render, "frame_%06d.png" % k), images[k, 0])
        summary["frames"] = int(images.shape[0])
        if renderer.mesh is not None:
            summary["robot_pixels"] = int((renderer.ids > 0).sum()) if images.shape[0] else 0
            renderer.mesh.close()
        print(f"wrote {images.shape[0]} frames to {a.render}; a video: ffmpeg -framerate "
              f"{1.0 / (float(env.dt) * a.render_every):g} -i {os.path.join(a.render, 'frame_%06d.png')} "
              "-pix_fmt yuv420p play.mp4")
    if sensor is not None:
        os.makedirs(a.depth, exist_ok=True)
        images = depth_frames.cpu().numpy()
        np.save(os.path.join(a.depth, "depth.npy"), images)
        near, far = sensor.near, sensor.far
        grey = np.floor(np.clip((far - images.astype(np.float32)) / (far - near), 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)
        for k in range(images.shape[0]):
            write_png(os.path.join(a.depth, "depth_%06d.png" % k), np.repeat(grey[k][:, :, None], 3, axis=2))
        summary["depth_frames"] = int(images.shape[0])
        print(f"wrote {images.shape[0]} depth images to {a.depth}")
    with open(os.path.join(a.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))
    return summary


if __name__ == "__main__":
    main()
