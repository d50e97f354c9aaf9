"""MI355X-native stand-in for the reference's `trainer.Trainer`
(/root/reference/code/trainer.py:17-384): same constructor, attributes and
forward / get_label_value / backprop signatures and return types, so
`from trainer import Trainer` (code/main.py:17) keeps working - but every network
evaluation, the Huber / cross-entropy loss, the backward pass and the Adam step run
in libsmg_hip.so (hand-written HIP for gfx950).

Differences that are deliberate and documented:
  * image_mean / image_std are constructor arguments (default 0.01 / 0.03); the
    released constants are [0,0,0] / [0,0,0] (code/trainer.py:176-177) which makes
    every network input inf/NaN.  `literal_reference=True` reproduces that.
  * the masked stream's trunk pass is computed once per sweep instead of once per
    rotation (code/models.py:385 sits inside the rotation loop); results are identical.
  * no CPU mode: without a GPU (or with force_cpu=True) the first forward raises.
"""
import copy
import os
import time

import numpy as np
import torch

import smg_hip
from models import STYLE_HEAD, STYLE_TRUNK, reactive_net, reinforcement_net

_ACTION_STYLE = {"grasp": 0, "suction": 1, "grasp_then_suction": 2}


def _f32_on(dev, a):
    """A host array or a tensor as a contiguous float32 tensor on `dev` (None stays None)."""
    if a is None:
        return None
    if torch.is_tensor(a):
        return a.to(device=dev, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _i32_on(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


class FusedAdam(object):
    """torch.optim.Adam(lr=1e-4, betas=(0.9,0.999), eps=1e-8, weight_decay=0)
    (code/trainer.py:99) over the model's flat parameter buffer.  Like torch >= 2
    (zero_grad(set_to_none=True)) only parameters that received a gradient in this
    step are updated: the engine reports which (trunk, head) segments those are."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
        self.model, self.lr, self.betas, self.eps = model, lr, betas, eps
        self.m = None
        self.v = None
        self.steps = {}

    def zero_grad(self, set_to_none=True):
        self.model.zero_grad()

    def _segments(self):
        if self.model._saved is None:
            return []
        _, _, trunk_id, head_id = self.model._saved
        return [("trunk%d" % trunk_id, smg_hip.trunk_range(self.model.HEAD_OUT, trunk_id)),
                ("head%d" % head_id, smg_hip.head_range(self.model.HEAD_OUT, head_id))]

    def step(self, segments=None):
        model = self.model
        p = model._flat_params
        if self.m is None or self.m.device != p.device:
            self.m = torch.zeros_like(p)
            self.v = torch.zeros_like(p)
        stream = torch.cuda.current_stream(p.device).cuda_stream
        for name, (off, n) in (segments if segments is not None else self._segments()):
            self.steps[name] = self.steps.get(name, 0) + 1
            smg_hip.adam_step(p.data_ptr(), model.flat_grads().data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                              off, n, self.steps[name], self.lr, self.betas[0], self.betas[1], self.eps, stream)


class Trainer(object):
    def __init__(self, method, future_reward_discount, load_snapshot, snapshot_file, force_cpu,
                 image_mean=0.01, image_std=0.03, literal_reference=False):
        self.method = method
        # code/trainer.py:22-31
        if torch.cuda.is_available() and not force_cpu:
            print("CUDA detected. Running with GPU acceleration.")
            self.use_cuda = True
        elif force_cpu:
            print("CUDA detected, but overriding with option '--cpu'. Running with only CPU.")
            self.use_cuda = False
        else:
            print("CUDA is *NOT* detected. Running with only CPU.")
            self.use_cuda = False
        self.image_mean = 0.0 if literal_reference else float(image_mean)
        self.image_std = 0.0 if literal_reference else float(image_std)

        if self.method == 'reactive':                                   # code/trainer.py:34-69
            self.model = reactive_net(self.use_cuda)
            if load_snapshot:
                self.model.load_state_dict(torch.load(snapshot_file))
                print('Pre-trained model snapshot loaded from: %s' % (snapshot_file))
            if self.use_cuda:
                self.model = self.model.cuda()
        elif self.method == 'reinforcement':                            # code/trainer.py:72-92
            self.model = reinforcement_net(self.use_cuda)
            self.model_target = copy.deepcopy(self.model)
            self.model_target.load_state_dict(self.model.state_dict())
            self.future_reward_discount = future_reward_discount
            if load_snapshot:
                self.model.load_state_dict(torch.load(snapshot_file))
                print('Pre-trained model snapshot loaded from: %s' % (snapshot_file))
            if self.use_cuda:
                self.model = self.model.cuda()
                self.model_target = self.model_target.cuda()
        else:
            raise ValueError("method must be 'reactive' or 'reinforcement'")

        self.model.train()                                              # code/trainer.py:95
        self.optimizer = FusedAdam(self.model)                          # code/trainer.py:99
        self.iteration = 0
        # code/trainer.py:105-114
        self.executed_action_log = []
        self.label_value_log = []
        self.reward_value_log = []
        self.predicted_value_log = []
        self.use_heuristic_log = []
        self.is_exploit_log = []
        self.clearance_log = []
        self.grasping_type_log = []
        self.episode_success_log = []
        self.training_loss_log = []

    # ---- session resume ---------------------------------------------------------------------
    # (file stem, attribute, layout): how code/trainer.py:118-160 re-reads each text log of a
    # previous session.  "rows" keeps the first `iteration` rows of a 2-D log, "col" the first
    # `iteration` entries of a 1-D log as an [iteration, 1] column, "col_all" every entry.
    _LOG_FILES = (
        ("executed-action", "executed_action_log", "rows"),
        ("label-value", "label_value_log", "col"),
        ("predicted-value", "predicted_value_log", "col"),
        ("reward-value", "reward_value_log", "col"),
        ("use-heuristic", "use_heuristic_log", "col"),
        ("is-exploit", "is_exploit_log", "col"),
        ("clearance", "clearance_log", "col_all"),
        ("grasping_type", "grasping_type_log", "col"),
        ("episode_success", "episode_success_log", "rows"),
        ("training_loss", "training_loss_log", "rows"),
    )

    def preload(self, transitions_directory):
        """code/trainer.py:118-160 (`--continue_logging`, code/main.py:74): reload the ten
        `<name>.log.txt` files of a logging session as python lists and resume the
        iteration counter at (rows of executed-action.log.txt) - 2."""
        def read(stem):
            return np.loadtxt(os.path.join(transitions_directory, stem + ".log.txt"), delimiter=" ")
        self.iteration = read("executed-action").shape[0] - 2
        n = self.iteration
        for stem, attr, how in self._LOG_FILES:
            a = read(stem)
            if how == "rows":
                a = a[0:n, :]
            elif how == "col":
                a = a[0:n].reshape(n, 1)
            else:
                a = a.reshape(a.shape[0], 1)
            setattr(self, attr, a.tolist())

    # ---- network evaluation -----------------------------------------------------------------
    def _heightmaps_to_device(self, depth_heightmap, m_depth_heightmap):
        hm = np.stack([np.asarray(depth_heightmap, dtype=np.float64), np.asarray(m_depth_heightmap, dtype=np.float64)])
        if hm.ndim != 3 or hm.shape[1] != hm.shape[2]:
            raise ValueError("heightmaps must be square 2-D arrays")
        dev = self.model._flat_params.device
        return torch.from_numpy(np.ascontiguousarray(hm)).to(dev)

    def _evaluate(self, model, depth_heightmap, m_depth_heightmap, style, is_volatile, specific_rotation):
        """Rotation selection of reinforcement_net.forward / reactive_net.forward
        (code/models.py:363-586) on the heightmap fast path: the x2 zoom, padding,
        3-channel replication and normalisation of code/trainer.py:165-191 happen inside
        the engine's input kernel."""
        model._require_gpu()
        hm = self._heightmaps_to_device(depth_heightmap, m_depth_heightmap)
        if is_volatile and specific_rotation == -1:
            if style == 0:
                rots, num = list(range(model.gnum_rotations)), model.gnum_rotations
            elif style == 1:
                rots, num = list(range(model.snum_rotations)), model.snum_rotations
            else:
                rots, num = [0], model.gnum_rotations
        else:
            rots, num = [0 if style == 2 else specific_rotation], model.gnum_rotations
        return model.run(style, rots, num, heightmaps=hm, mean=self.image_mean, std=self.image_std,
                         keep_for_backward=not is_volatile)

    def forward(self, depth_heightmap, m_depth_heightmap, style=0, is_volatile=False, is_target=False, specific_rotation=-1):
        """code/trainer.py:162-209.  Returns np.ndarray float64 of length R (reinforcement)
        or a python float P(success) (reactive, :195-199)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.method == 'reactive':
                q = self._evaluate(self.model, depth_heightmap, m_depth_heightmap, style, is_volatile, specific_rotation)
                self._last_q = q
                logits = q[0].reshape(1, 3, 1, 1)
                return torch.softmax(logits, dim=1).cpu().numpy()[0, 0, 0][0]
            model = self.model_target if is_target else self.model
            q = self._evaluate(model, depth_heightmap, m_depth_heightmap, style, is_volatile, specific_rotation)
            self._last_q = q
            if q.shape[2] * q.shape[3] != 1:
                raise NotImplementedError("dense Q maps (input larger than 640) cannot be returned through the "
                                          "reference's scalar-per-rotation array (code/trainer.py:205-207)")
            return q.reshape(-1).cpu().numpy().astype(np.float64)

    def _objects_on_device(self, model, depth_heightmap, mask_depth):
        dev = model._flat_params.device
        d = torch.from_numpy(np.ascontiguousarray(np.asarray(depth_heightmap, dtype=np.float64))[None]).to(dev)
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(mask_depth, dtype=np.float64))).to(dev)
        if m.ndim != 3 or m.shape[1:] != d.shape[1:]:
            raise ValueError("mask_depth must be [n_objects, H, H] like the heightmap")
        return d, m

    def _object_maps(self, what, depth_heightmap, mask_depth, style, is_target):
        """The one engine call behind forward_objects, forward_objects_dense and forward_class_objects, with its BN sequence:
        -> (model, q [n * R, HEAD_OUT, OH, OW] object-major, the masks on the device, n, R).  The caller checks the method."""
        if style not in (0, 1):
            raise ValueError("%s: styles 0 (grasp) and 1 (suction)" % what)
        model = self.model_target if is_target else self.model
        d, m = self._objects_on_device(model, depth_heightmap, mask_depth)
        n = int(m.shape[0])
        R = model.gnum_rotations if style == 0 else model.snum_rotations
        pairs = [(r, k) for k in range(n) for r in range(R)]
        seq_t = [v for k in range(n) for r in range(R) for v in (r, R + k)]       # trunk(rot r), trunk(mask k) per sample
        q = model.run_pairs(style, R, d, list(range(R)), [0] * n, pairs, self.image_mean, self.image_std,
                            bn_seq_trunk=seq_t, bn_seq_head=list(range(len(pairs))),
                            masks=m, mask_a=list(range(n)), mask_b=[-1] * n)
        return model, q, m, n, R

    def forward_objects(self, depth_heightmap, mask_depth, style=0, is_target=False, return_device=False):
        """All objects of one scene in ONE engine call - the loop of code/main.py:158-166:

            for num in range(objects_number):
                gra_conf[num] = trainer.forward(depth, depth * mask_depth[num], style, is_volatile=True)

        The rotated full-depth streams are the same for every object, so n objects x R rotations
        cost R + n trunk passes (the reference runs 2*n*R).  The products depth * mask[k] are formed
        on the device by the input kernel (the host ships the heightmap and the masks once).  BN
        running statistics are updated in the reference's order and count.
        Returns conf[n_objects, R] float64 (styles 0 / 1), or the device tensor [n*R] if asked."""
        if self.method != 'reinforcement':
            raise ValueError("forward_objects: reinforcement method only (the reactive net's form is forward_class_objects)")
        _, q, _, n, R = self._object_maps("forward_objects", depth_heightmap, mask_depth, style, is_target)
        if q.shape[2] * q.shape[3] != 1:
            raise NotImplementedError("dense Q maps")
        if return_device:
            return q.reshape(-1)
        return q.reshape(n, R).cpu().numpy().astype(np.float64)

    def _object_pair_maps(self, depth_heightmap, mask_depth, is_target):
        """The one engine call behind forward_object_pairs, forward_object_pairs_dense and forward_class_object_pairs, with its BN
        sequence: style 2, rotation 0, the mask of pair (g < s) = mask[g] + mask[s] -> (model, q [n_pairs, HEAD_OUT, OH, OW], the masks on the device, [(g, s)]); q
        and the masks are None without a pair (nothing runs)."""
        model = self.model_target if is_target else self.model
        n = int(np.asarray(mask_depth).shape[0])
        idx = [(g, s) for g in range(n) for s in range(g + 1, n)]
        if not idx:
            return model, None, None, idx
        d, m = self._objects_on_device(model, depth_heightmap, mask_depth)
        pairs = [(0, k) for k in range(len(idx))]
        seq_t = [v for k in range(len(idx)) for v in (0, 1 + k)]
        q = model.run_pairs(2, model.gnum_rotations, d, [0], [0] * len(idx), pairs, self.image_mean, self.image_std,
                            bn_seq_trunk=seq_t, bn_seq_head=list(range(len(idx))),
                            masks=m, mask_a=[g for g, _ in idx], mask_b=[s_ for _, s_ in idx])
        return model, q, m, idx

    def forward_object_pairs(self, depth_heightmap, mask_depth, is_target=False, return_device=False):
        """The enveloping-then-sucking loop of code/main.py:183-192 in one engine call: for every
        unordered object pair (g < s) the mask is mask[g] + mask[s] (summed and applied on the device),
        style 2, rotation 0.  Returns gs_conf[n, n] with -100 where the reference leaves its fill value
        (main.py:184), or (device tensor of the pair values, [(g, s)]) if asked."""
        n = int(np.asarray(mask_depth).shape[0])
        gs = np.full((n, n), -100.0)
        _, q, _, idx = self._object_pair_maps(depth_heightmap, mask_depth, is_target)
        if not idx:
            return (None, idx) if return_device else gs
        if return_device:
            return q.reshape(-1), idx
        vals = q.reshape(-1).cpu().numpy().astype(np.float64)
        for (g, s), v in zip(idx, vals):
            gs[g, s] = v
        return gs

    def best_actions(self, depth_heightmap, mask_depth, is_ets=True):
        """The whole per-step evaluation of code/main.py:158-195 - grasp and suction sweeps over every object, the ES
        pass over every object pair, and the three np.argmax selections - in three engine calls whose maxima are
        found on the device (smg_argmax: lowest index on ties, like np.argmax); the host reads back three
        (index, value) pairs instead of 2*n*R + n(n-1)/2 scalars.
        Returns bestg_id / bests_id = (object, rotation), bestg_conf / bests_conf, and for ES bestgs_num = (g, s),
        bestgs_conf (None / 0 with fewer than two objects, main.py:180-183)."""
        model = self.model
        dev = model._flat_params.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        idx = torch.empty(3, dtype=torch.int32, device=dev)
        val = torch.zeros(3, dtype=torch.float32, device=dev)
        R = (model.gnum_rotations, model.snum_rotations)
        for style in (0, 1):
            q = self.forward_objects(depth_heightmap, mask_depth, style, return_device=True)
            smg_hip.argmax(q.data_ptr(), q.numel(), idx[style:].data_ptr(), val[style:].data_ptr(), stream)
        pair_list = []
        if is_ets and np.asarray(mask_depth).shape[0] > 1:
            q, pair_list = self.forward_object_pairs(depth_heightmap, mask_depth, return_device=True)
            smg_hip.argmax(q.data_ptr(), q.numel(), idx[2:].data_ptr(), val[2:].data_ptr(), stream)
        i, v = idx.cpu().numpy(), val.cpu().numpy().astype(np.float64)
        out = {"bestg_id": (int(i[0]) // R[0], int(i[0]) % R[0]), "bestg_conf": v[0],
               "bests_id": (int(i[1]) // R[1], int(i[1]) % R[1]), "bests_conf": v[1],
               "bestgs_num": None, "bestgs_conf": 0}
        if pair_list:
            out["bestgs_num"], out["bestgs_conf"] = pair_list[int(i[2])], v[2]
        return out

    @staticmethod
    def _class_label(primitive_action, suction_success, grasp_success, gs_success):
        """The reactive label of code/trainer.py:214-232, which needs no network: (label_value, success_value), printed."""
        label_value = 0
        if primitive_action == 'suction':
            success_value = suction_success
            if not suction_success:
                label_value = 1
        elif primitive_action == 'grasp':
            success_value = grasp_success
            if not grasp_success:
                label_value = 1
        elif primitive_action == 'grasp_then_suction':
            success_value = gs_success
            label_value = 0 if gs_success == 2.5 else 1
        print('Label value: %d' % (label_value))
        return label_value, success_value

    @staticmethod
    def _reward_now(primitive_action, objects_number, suction_success, grasp_success, gs_success):
        """The part of code/trainer.py:236-253 that needs no network: (current_reward, whether the future reward is 0 - nothing
        succeeded, or the scene is cleared)."""
        current_reward = 0
        if primitive_action == 'suction':
            current_reward = suction_success
        elif primitive_action == 'grasp':
            current_reward = grasp_success
        elif primitive_action == 'grasp_then_suction':
            current_reward = gs_success
        if suction_success == 0 and grasp_success == 0 and gs_success == 0:
            return current_reward, True
        return current_reward, bool((objects_number == 1 and suction_success == 1) or (objects_number == 1 and grasp_success == 1) or
                                    (objects_number == 2 and gs_success == 2.5))

    def get_label_value(self, primitive_action, objects_number,
                        suction_success, grasp_success, gs_success,
                        depth_heightmap, mask_depth, objects_mask,
                        bestg_id, bests_id, bestgs_g_id, bestgs_s_id,
                        exploit_action, bestg_conf, bests_conf, bestgs_conf):
        """code/trainer.py:212-274."""
        if self.method == 'reactive':
            return self._class_label(primitive_action, suction_success, grasp_success, gs_success)
        current_reward, no_future = self._reward_now(primitive_action, objects_number, suction_success, grasp_success, gs_success)
        if no_future:
            future_reward = 0
        else:
            if exploit_action == 'grasp':
                m = depth_heightmap * mask_depth[bestg_id[0]]
                future_reward = self.forward(depth_heightmap, m, style=0, is_volatile=True, is_target=True, specific_rotation=bestg_id[1])[0]
            elif exploit_action == 'suction':
                m = depth_heightmap * mask_depth[bests_id[0]]
                future_reward = self.forward(depth_heightmap, m, style=1, is_volatile=True, is_target=True, specific_rotation=bests_id[1])[0]
            elif exploit_action == 'grasp_then_suction':
                m = depth_heightmap * (mask_depth[bestgs_g_id[0]] + mask_depth[bestgs_s_id[0]])
                future_reward = self.forward(depth_heightmap, m, style=2, is_volatile=True, is_target=True, specific_rotation=bestgs_g_id[1])[0]
        expected_reward = current_reward + self.future_reward_discount * future_reward
        print('Expected reward: %f + %f x %f = %f' % (current_reward, self.future_reward_discount, future_reward, expected_reward))
        return expected_reward, current_reward

    def backprop(self, depth_heightmap, primitive_action,
                 bestg_id, bests_id, bestgs_g_id, bestgs_s_id,
                 label_value, objects_mask, sro_best, gro_best, bestgs_num):
        """code/trainer.py:278-384: one sample, one optimizer step; returns a 0-d array."""
        mask_depth = objects_mask.copy()
        objects_mask.shape = (objects_mask.shape[0], objects_mask.shape[1], objects_mask.shape[2], 1)   # trainer.py:288,336
        style = _ACTION_STYLE[primitive_action]
        if style == 0:
            m = depth_heightmap * mask_depth[bestg_id[0]]
            rot = bestg_id[1]
        elif style == 1:
            m = depth_heightmap * mask_depth[bests_id[0]]
            rot = bests_id[1]
        else:
            m = depth_heightmap * (mask_depth[bestgs_g_id[0]] + mask_depth[bestgs_s_id[0]])
            rot = bestgs_g_id[1]
        loss_value = self.train_step(depth_heightmap, m, style, rot, label_value)
        print('Training loss: %f' % (loss_value))
        return loss_value

    def _scenes_to_device(self, depth_heightmap, m_depth_heightmap, rotations):
        """The (depth, masked depth) heightmaps of one scene (2-D) or several ([n_scenes, H, H]) as the interleaved device tensor
        [2 * n_scenes, H, H] float64 that model.run reads, and `rotations` as one list per scene."""
        if torch.is_tensor(depth_heightmap) and depth_heightmap.is_cuda:
            # device-resident inputs (float64 heightmaps, float32 labels): nothing crosses PCIe and - unlike a pageable
            # host-to-device copy - nothing makes the host wait for the previous step's kernels
            d = depth_heightmap.to(dtype=torch.float64)
            m = m_depth_heightmap.to(device=d.device, dtype=torch.float64)
            if d.dim() == 2:
                d, m, rotations = d[None], m[None], [list(rotations)]
            hm = torch.stack((d, m), dim=1).reshape((2 * d.shape[0],) + tuple(d.shape[1:])).contiguous()
        else:
            d = np.asarray(depth_heightmap, dtype=np.float64)
            m = np.asarray(m_depth_heightmap, dtype=np.float64)
            if d.ndim == 2:
                d, m, rotations = d[None], m[None], [list(rotations)]
            hm = np.empty((2 * d.shape[0],) + d.shape[1:], dtype=np.float64)
            hm[0::2], hm[1::2] = d, m
            hm = torch.from_numpy(hm).to(self.model._flat_params.device)
        return hm, rotations

    def train_batch(self, depth_heightmap, m_depth_heightmap, style, rotations, labels, grad_sync=None, return_q=False):
        """Batched form of backprop: every (scene, rotation) is a training sample (forward as
        branch C, Huber / CE against its label); the gradient of the SUM of the losses is
        accumulated in one backward pass (each scene's masked stream is walked once with the summed
        gradient - exact, the trunk is linear in its output gradient), then ONE Adam step.  Equals
        that many reference backprop calls with the optimizer step deferred to the end.

        One scene: 2-D heightmaps, `rotations` a list of rotation indices.  Several scenes
        (SURVEY.md config 4): heightmaps [n_scenes, H, H], `rotations` a list of lists; labels are
        flat, scene-major.  `grad_sync(model, trunk_id, head_id)` is the data-parallel hook
        (parallel.allreduce_grads) called between backward and Adam; a hook with `.overlapped` set (parallel.OverlappedGradSync)
        gets `.start()` after the first half of the backward and `.finish()` after the second.  Returns the loss vector."""
        model = self.model
        self.optimizer.zero_grad()
        model._require_gpu()
        hm, rotations = self._scenes_to_device(depth_heightmap, m_depth_heightmap, rotations)
        num = model.gnum_rotations                     # code/models.py:522,545,568 (gnum for every style)
        rots = [[0 if style == 2 else int(r) for r in rs] for rs in rotations]
        dev = model._flat_params.device
        if torch.is_tensor(labels):
            lab = labels.to(device=dev, dtype=torch.float32).reshape(-1)
        else:      # (uploaded BEFORE the forward is enqueued: behind it, the pageable copy would hold the host until the forward has run)
            lab_h = np.asarray(labels, dtype=np.float32).reshape(-1)
            if self.method == 'reactive' and not np.isin(lab_h, (0.0, 1.0, 2.0)).all():
                # torch's nll_loss (code/utils.py:311) raises on a class index outside [0, 3); the loss kernel would
                # silently treat it as the weight-0 class.  (Device-resident labels are not read back: same contract.)
                raise ValueError("reactive labels must be class indices 0, 1 or 2")
            lab = torch.as_tensor(lab_h, device=dev)
        q = model.run(style, rots, num, heightmaps=hm, mean=self.image_mean, std=self.image_std, keep_for_backward=True)
        n = q.shape[0]
        eng, token, trunk_id, head_id = model._saved
        stream = torch.cuda.current_stream(dev).cuda_stream
        if lab.numel() != n:
            raise ValueError("one label per (scene, rotation) sample")
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        dq = torch.empty_like(q)
        eng.loss(0 if self.method == 'reinforcement' else 1, q.data_ptr(), lab.data_ptr(), n, loss.data_ptr(), dq.data_ptr(), stream)
        self._backward_and_step(token, dq, trunk_id, head_id, grad_sync)
        return (loss, q) if return_q else loss

    def _backward_and_step(self, token, dq, trunk_id, head_id, grad_sync):
        model = self.model
        if grad_sync is not None and getattr(grad_sync, "overlapped", False):
            # the all-reduce of everything behind dense block 1 (most of the parameters) runs under the second half of the backward
            model._engine_backward(token, dq, phase=0)
            grad_sync.start(model, trunk_id, head_id)
            model._engine_backward(token, dq, phase=1)
            grad_sync.finish(model, trunk_id, head_id)
        else:
            model._engine_backward(token, dq)
            if grad_sync is not None:
                grad_sync(model, trunk_id, head_id)
        self.optimizer.step()

    # ---- dense Q maps (heightmaps larger than 224^2: one Q value per 20x20 window of the feature plane) ------------------------
    @staticmethod
    def dense_map_size(heightmap_size):
        """Side OH = OW of the Q map of a heightmap_size^2 heightmap: the padded input (code/trainer.py:165-173) through the
        DenseNet-121 strides (stem conv, pool0, three transitions) and the head's 20x20 valid convolution.  224 -> 1, 240 -> 3,
        320 -> 10, 640 -> 38."""
        hm = int(heightmap_size)
        diag = np.ceil(float(2 * hm) * np.sqrt(2) / 32) * 32
        n = 2 * hm + 2 * int((diag - 2 * hm) / 2)
        n = (n - 1) // 2 + 1          # conv0: 7x7, stride 2, padding 3
        n = (n - 1) // 2 + 1          # pool0: 3x3, stride 2, padding 1
        for _ in range(3):
            n //= 2                   # transition average pools
        return n - 20 + 1

    def forward_dense(self, depth_heightmap, m_depth_heightmap, style=0, is_target=False, specific_rotation=-1, return_device=False):
        """Trainer.forward(..., is_volatile=True) without the scalar-per-rotation restriction: the whole Q map of every evaluated
        rotation, float64 [R, OH, OW] (R rows from the sweep, 1 from a specific rotation or style 2) - or the float32 device
        tensor of that shape if asked.  Rotation choice and BN bookkeeping are forward's; a 224^2 heightmap gives [R, 1, 1] with
        forward's values.  Reinforcement method only (the reactive head's output is a class distribution, not a map of values)."""
        if self.method != 'reinforcement':
            raise ValueError("forward_dense: reinforcement method only")
        model = self.model_target if is_target else self.model
        with np.errstate(divide="ignore", invalid="ignore"):
            q = self._evaluate(model, depth_heightmap, m_depth_heightmap, style, True, specific_rotation)
        self._last_q = q
        q = q.reshape(q.shape[0], q.shape[2], q.shape[3])
        return q if return_device else q.cpu().numpy().astype(np.float64)

    def best_dense_action(self, depth_heightmap, m_depth_heightmap, style=0, is_target=False):
        """The best (rotation, pixel) of the sweep's dense Q maps, found on the device (smg_argmax over the flattened [R, OH, OW]:
        lowest index on ties like np.argmax, a NaN wins); the host reads back one (index, value) pair.
        Returns {"rotation", "pixel": (oy, ox), "conf"}."""
        q = self.forward_dense(depth_heightmap, m_depth_heightmap, style, is_target, return_device=True)
        dev = q.device
        idx = torch.empty(1, dtype=torch.int32, device=dev)
        val = torch.empty(1, dtype=torch.float32, device=dev)
        smg_hip.argmax(q.data_ptr(), q.numel(), idx.data_ptr(), val.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        i = int(idx.cpu().numpy()[0])
        _, OH, OW = q.shape
        return {"rotation": i // (OH * OW), "pixel": ((i // OW) % OH, i % OW), "conf": float(val.cpu().numpy().astype(np.float64)[0])}

    def train_batch_maps(self, depth_heightmap, m_depth_heightmap, style, rotations, label_maps, weight_maps=None, grad_sync=None, return_q=False):
        """train_batch with a whole label map per sample - the per-pixel formulation: the loss of sample j is
        sum over its Q map of weight * Huber(q - label) (smg_loss_map; `weight_maps` None = all ones, a weight of 0 masks its
        pixel), the gradient of the SUM of the losses goes back in one backward pass - the head's value convolution in its dense
        form - and ONE Adam step follows.  Scenes, rotations, host or device inputs and `grad_sync` as in train_batch;
        `label_maps` / `weight_maps` are [n_samples, OH, OW] (dense_map_size), scene-major.  Reinforcement method only.
        Returns the loss vector (and q [n_samples, 1, OH, OW] if asked)."""
        if self.method != 'reinforcement':
            raise ValueError("train_batch_maps: reinforcement method only (a map of Q values; the reactive head is a classifier)")
        n = len(self._flat_rotations(depth_heightmap, style, rotations))
        side = self.dense_map_size(np.shape(depth_heightmap)[-1])
        for name, maps in (("label_maps", label_maps), ("weight_maps", weight_maps)):
            if maps is not None and tuple(maps.shape if torch.is_tensor(maps) else np.shape(maps)) != (n, side, side):
                raise ValueError("%s must be [%d samples, %d, %d] for a %d^2 heightmap, got %s"
                                 % (name, n, side, side, np.shape(depth_heightmap)[-1], tuple(np.shape(maps))))

        def loss_call(eng, q, tensors, n, loss, dq, stream):
            eng.loss_map(q.data_ptr(), _ptr(tensors[0]), _ptr(tensors[1]), n, loss.data_ptr(), dq.data_ptr(), stream)
        return self._train_maps(depth_heightmap, m_depth_heightmap, style, rotations, (1, side),
                                lambda dev: (_f32_on(dev, label_maps), _f32_on(dev, weight_maps)), loss_call, grad_sync, return_q)

    @staticmethod
    def _flat_rotations(depth_heightmap, style, rotations):
        """The rotation of every sample as one flat list, scene-major (`rotations` is a list per scene where the heightmaps are
        [n_scenes, H, H]); style 2 is rotation 0."""
        flat = [r for rs in rotations for r in rs] if np.ndim(depth_heightmap) == 3 else list(rotations)
        return [0 if style == 2 else int(r) for r in flat]

    def _train_maps(self, depth_heightmap, m_depth_heightmap, style, rotations, q_shape, upload, loss_call, grad_sync, return_q, n_loss=None):
        """The step that train_batch_maps, train_batch_class_maps and the four train_batch_scene_* methods share, entered once their
        own arguments are checked: the forward of every (scene, rotation) sample kept for the backward, ONE engine loss call on its
        q [n, channels, side, side] (`q_shape` = the expected (channels, side)), one backward pass, ONE Adam step.
        `upload(dev)` returns the device tensors of the labels and is called BEFORE the forward is enqueued (behind it, a pageable
        copy would hold the host until the forward has run); `loss_call(eng, q, tensors, n, loss, dq, stream)` enqueues the loss
        that fills loss [n] - or [n_loss] where the loss is not per sample (train_batch_scene_policy's is per group) - and dq (shaped
        like q).  Returns the loss vector (and q if asked)."""
        model = self.model
        self.optimizer.zero_grad()
        model._require_gpu()
        dev = model._flat_params.device
        hm, rotations = self._scenes_to_device(depth_heightmap, m_depth_heightmap, rotations)
        rots = [[0 if style == 2 else int(r) for r in rs] for rs in rotations]
        n = sum(len(rs) for rs in rots)
        tensors = upload(dev)
        q = model.run(style, rots, model.gnum_rotations, heightmaps=hm, mean=self.image_mean, std=self.image_std, keep_for_backward=True)
        eng, token, trunk_id, head_id = model._saved
        assert tuple(q.shape) == (n, q_shape[0], q_shape[1], q_shape[1]), (tuple(q.shape), n, q_shape)
        stream = torch.cuda.current_stream(dev).cuda_stream
        loss = torch.empty(n if n_loss is None else n_loss, dtype=torch.float32, device=dev)
        dq = torch.empty_like(q)
        loss_call(eng, q, tensors, n, loss, dq, stream)
        self._backward_and_step(token, dq, trunk_id, head_id, grad_sync)
        return (loss, q) if return_q else loss

    def train_batch_pixels(self, depth_heightmap, m_depth_heightmap, style, rotations, pixels, labels, grad_sync=None, return_q=False):
        """train_batch_maps with ONE trained pixel per sample: `pixels` holds an (oy, ox) per sample, `labels` its target value -
        expressed as a one-hot weight map with the label at that pixel.  Pixel (0, 0) is the element train_batch trains."""
        lab = np.asarray(labels, dtype=np.float32).reshape(-1)
        pix = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
        side = self.dense_map_size(np.shape(depth_heightmap)[-1])
        if len(pix) != len(lab):
            raise ValueError("one (oy, ox) and one label per sample")
        if len(pix) and (pix.min() < 0 or pix.max() >= side):
            raise ValueError("pixels must lie inside the %d x %d Q map" % (side, side))
        label_maps = np.zeros((len(lab), side, side), dtype=np.float32)
        weight_maps = np.zeros_like(label_maps)
        k = np.arange(len(lab))
        label_maps[k, pix[:, 0], pix[:, 1]] = lab
        weight_maps[k, pix[:, 0], pix[:, 1]] = 1.0
        return self.train_batch_maps(depth_heightmap, m_depth_heightmap, style, rotations, label_maps, weight_maps, grad_sync, return_q)

    # ---- dense Q maps in the scene frame: rotated back and bilinearly upsampled onto the heightmap's pixels ---------------------------
    @staticmethod
    def _scene_geometry(heightmap_size):
        """(pad, S, side) of a heightmap_size^2 heightmap (code/trainer.py:165-173); ValueError where the Q map is 1 x 1."""
        hm = int(heightmap_size)
        pad = int((np.ceil(float(2 * hm) * np.sqrt(2) / 32) * 32 - 2 * hm) / 2)
        S = 2 * hm + 2 * pad
        side = S // 32 - 19
        if side < 2:
            raise ValueError("a %d^2 heightmap gives a %d x %d Q map: nothing to interpolate over (the scene-frame interface "
                             "needs a heightmap larger than 224^2)" % (hm, side, side))
        return pad, S, side

    @staticmethod
    def scene_to_map(heightmap_size, rotation, num_rotations, pixels):
        """Where heightmap pixels lie on the dense Q map of `rotation` (of `num_rotations`): `pixels` [..., 2] = (iy, ix) ->
        (qy, qx, valid), float64 map coordinates and whether a window of the head is centred there (0 <= q <= side - 1 on both
        axes).  `rotation` is one index or an array that broadcasts against pixels[..., 0].  The chain of include/smg_hip.h in
        float64 on the host: pixel -> centre of its 2x2 block of the padded input -> align_corners=True normalisation -> A^T u with
        A the 2x2 part of models.rotation_theta (the float32 numbers the forward samples with) -> input pixels -> (p - 319.5) / 32."""
        from models import rotation_theta
        pad, S, side = Trainer._scene_geometry(heightmap_size)
        pix = np.asarray(pixels)
        if pix.shape[-1:] != (2,):
            raise ValueError("pixels must be [..., 2] = (iy, ix)")
        rot = np.broadcast_to(np.asarray(rotation), pix.shape[:-1])
        A = np.zeros(pix.shape[:-1] + (4,), dtype=np.float64)
        for r in np.unique(rot):
            th = rotation_theta(int(r), num_rotations).astype(np.float64)
            A[rot == r] = (th[0], th[1], th[3], th[4])
        x = 2.0 * pix[..., 1].astype(np.float64) + 0.5 + pad
        y = 2.0 * pix[..., 0].astype(np.float64) + 0.5 + pad
        ux, uy = 2.0 * x / (S - 1) - 1.0, 2.0 * y / (S - 1) - 1.0
        px = (A[..., 0] * ux + A[..., 2] * uy + 1.0) / 2.0 * (S - 1)
        py = (A[..., 1] * ux + A[..., 3] * uy + 1.0) / 2.0 * (S - 1)
        qx, qy = (px - 319.5) / 32.0, (py - 319.5) / 32.0
        valid = (qx >= 0) & (qx <= side - 1) & (qy >= 0) & (qy <= side - 1)
        return qy, qx, valid

    def _require_scene(self, what, depth_heightmap):
        if self.method != 'reinforcement':
            raise ValueError("%s: reinforcement method only" % what)
        return self._scene_geometry(np.shape(depth_heightmap)[-1])

    def _scene_rotations(self, model, style, specific_rotation):
        """The (rotation, num_rotations) of every row of forward_dense's result, in _evaluate's order."""
        if specific_rotation == -1 and style == 0:
            return [(r, model.gnum_rotations) for r in range(model.gnum_rotations)]
        if specific_rotation == -1 and style == 1:
            return [(r, model.snum_rotations) for r in range(model.snum_rotations)]
        return [(0 if style == 2 else specific_rotation, model.gnum_rotations)]

    def forward_scene(self, depth_heightmap, m_depth_heightmap, style=0, is_target=False, specific_rotation=-1, return_device=False):
        """forward_dense in the SCENE frame: every evaluated rotation's Q map rotated back and bilinearly upsampled onto the
        heightmap's pixels (smg_scene_maps), float64 [R, hm, hm] - or the float32 device tensor - with -inf where no window of
        the head is centred in that rotation.  Element [r, iy, ix] is the Q value of acting at heightmap pixel (iy, ix) with
        rotation r: the same scene point in every rotation.  Rotation choice and BN bookkeeping are forward's (style 2 is
        rotation 0).  Reinforcement method, heightmaps larger than 224^2."""
        self._require_scene("forward_scene", depth_heightmap)
        model = self.model_target if is_target else self.model
        q = self.forward_dense(depth_heightmap, m_depth_heightmap, style, is_target, specific_rotation, return_device=True)
        R, OH, OW = q.shape
        eng, aff, hm, stream = self._scene_call(model, q, depth_heightmap, self._scene_rotations(model, style, specific_rotation))
        out = torch.empty((R, hm, hm), dtype=torch.float32, device=q.device)
        eng.scene_maps(q.data_ptr(), OH * OW, R, aff, hm, out.data_ptr(), stream)
        return out if return_device else out.cpu().numpy().astype(np.float64)

    def _scene_call(self, model, q, depth_heightmap, rots):
        """(engine, affine matrices, hm, stream) of a scene-frame call on the maps q of the `rots` = [(rotation, num_rotations)]."""
        import models
        assert len(rots) == q.shape[0]
        hm = int(np.shape(depth_heightmap)[-1])
        eng = models.get_engine(q.device.index or 0, self._scene_geometry(hm)[1], model.HEAD_OUT, 1, 1)
        return eng, [models.rotation_theta(r, num) for r, num in rots], hm, torch.cuda.current_stream(q.device).cuda_stream

    def _best_scene(self, q, hm, rots, argmax):
        """`argmax(idx_ptr, val_ptr)` enqueues a scene argmax over the flattened [R, hm, hm]; the host reads back its one
        (index, value) pair.  Returns {"rotation", "pixel": (iy, ix), "conf", "map_pixel": (qy, qx)}."""
        idx = torch.empty(1, dtype=torch.int32, device=q.device)
        val = torch.empty(1, dtype=torch.float32, device=q.device)
        argmax(idx.data_ptr(), val.data_ptr())
        i = int(idx.cpu().numpy()[0])
        row, iy, ix = i // (hm * hm), (i // hm) % hm, i % hm
        qy, qx, _ = self.scene_to_map(hm, rots[row][0], rots[row][1], (iy, ix))
        return {"rotation": rots[row][0], "pixel": (iy, ix), "conf": float(val.cpu().numpy().astype(np.float64)[0]),
                "map_pixel": (float(qy), float(qx))}

    def best_scene_action(self, depth_heightmap, m_depth_heightmap, style=0, is_target=False):
        """The best (rotation, heightmap pixel) of the sweep, found on the device without materialising the scene-frame maps
        (smg_scene_argmax: lowest index of the flattened [R, hm, hm] on ties like np.argmax, a NaN wins, pixels without a window
        are never picked); the host reads back one (index, value) pair.
        Returns {"rotation", "pixel": (iy, ix), "conf", "map_pixel": (qy, qx)} - `pixel` in heightmap pixels, `map_pixel` its
        float position on that rotation's Q map (scene_to_map)."""
        self._require_scene("best_scene_action", depth_heightmap)
        model = self.model_target if is_target else self.model
        q = self.forward_dense(depth_heightmap, m_depth_heightmap, style, is_target, return_device=True)
        R, OH, OW = q.shape
        rots = self._scene_rotations(model, style, -1)
        eng, aff, hm, stream = self._scene_call(model, q, depth_heightmap, rots)
        return self._best_scene(q, hm, rots, lambda idx, val: eng.scene_argmax(q.data_ptr(), OH * OW, R, aff, hm, idx, val, stream))

    def forward_objects_dense(self, depth_heightmap, mask_depth, style=0, is_target=False, return_device=False):
        """forward_objects on a heightmap larger than 224^2: its one engine call, with its BN sequence, and the whole Q map of every
        (object, rotation) kept - float64 [n_objects, R, OH, OW], or the float32 device tensor of that shape if asked.  The maps
        are in the rotated frame of their rotation, like forward_dense's."""
        self._require_scene("forward_objects_dense", depth_heightmap)
        _, q, _, n, R = self._object_maps("forward_objects_dense", depth_heightmap, mask_depth, style, is_target)
        q = q.reshape(n, R, q.shape[2], q.shape[3])
        return q if return_device else q.cpu().numpy().astype(np.float64)

    def forward_object_pairs_dense(self, depth_heightmap, mask_depth, is_target=False, return_device=False):
        """forward_object_pairs on a heightmap larger than 224^2: its one engine call, with its BN sequence, and the style-2 map of
        every object pair kept.  Returns (maps float64 [n_pairs, OH, OW] - or the float32 device tensor -, [(g, s)]); with fewer
        than two objects nothing runs and the maps are [0, OH, OW]."""
        _, _, side = self._require_scene("forward_object_pairs_dense", depth_heightmap)
        model, q, _, idx = self._object_pair_maps(depth_heightmap, mask_depth, is_target)
        if q is None:
            dev = model._flat_params.device
            q = torch.empty((0, side, side), dtype=torch.float32, device=dev if return_device else "cpu")
        else:
            q = q.reshape(len(idx), q.shape[2], q.shape[3])
        return (q if return_device else q.cpu().numpy().astype(np.float64)), idx

    def best_scene_actions(self, depth_heightmap, mask_depth, is_ets=True, is_target=False):
        """best_actions in the SCENE frame, for a heightmap larger than 224^2 - the whole per-step evaluation of code/main.py:158-195
        with every object's Q maps rotated back onto the heightmap and read on that object's OWN pixels (mask_depth[k] != 0; for
        the enveloping-then-sucking pair (g, s) the pixels of either object).  One engine forward per primitive and one
        smg_scene_argmax_objects on the masks tensor that forward used: per object (per pair) the best selected pixel with a window
        of the head over all its rotations, found on the device without writing the n * R scene-frame maps; the host reads back one
        (index, value) pair per object and primitive.  The overall best of a primitive is np.argmax over the objects' values (the
        first NaN wins, then the largest value, the lowest object on ties).
        Returns bestg_id / bests_id = (object, rotation), bestg_pixel / bests_pixel = (iy, ix), bestg_conf / bests_conf - None ids
        and pixels and -inf when no object has a selected pixel with a window -; bestgs_num = (g, s), bestgs_pixel, bestgs_conf
        (None / None / 0 with fewer than two objects or is_ets False, as in best_actions); per_object = {"grasp": [...],
        "suction": [...]}, one (rotation, (iy, ix), conf) per object or None.  is_target evaluates the target net (the future
        reward of get_label_value in this frame)."""
        self._require_scene("best_scene_actions", depth_heightmap)

        def argmax(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, idx, val, stream, style):
            eng.scene_argmax_objects(q.data_ptr(), q.shape[2] * q.shape[3], n_maps, aff, hm, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                     group_of, groups, idx, val, stream)
        return self._best_scene_objects("best_scene_actions", depth_heightmap, mask_depth, is_ets, is_target, argmax)

    def _scene_object_picks(self, what, depth_heightmap, mask_depth, is_ets, is_target, pick, k=1, joint=False, stats=None, betas=()):
        """The loop behind best_scene_actions, ranked_scene_actions, sampled_scene_actions and their class forms (the caller has
        checked method and geometry): one forward per primitive, one pick(engine, q, n_maps, affines, hm, masks, mask_a, mask_b,
        group of every map, n_groups, idx pointer, val pointer, stream, style) on its maps - which writes `k` (index, value) pairs
        per group - and one read-back.  The groups are the objects (the pairs), or with `joint` ONE group of all the primitive's
        maps.  Returns (calls = per primitive (first group, groups, maps per object), indices [all groups, k], values float64
        [all groups, k], the pair list or None, hm, statistics); the maps behind the result stay in self._last_object_q.
        `stats` (scene_policy_stats, and the sampled forms' with_stats): after the pick, one stats(engine, q, n_maps, affines, hm,
        masks, mask_a, mask_b, group of every map, n_groups, row pointer, stream, beta) per entry of `betas` on the same maps and
        masks, enqueued before the read-back; statistics = float64 [len(betas), all groups, 4] = {count, vmax, lse, mean}, else
        None.  `pick` None: the statistics alone (indices and values are None)."""
        n = int(np.asarray(mask_depth).shape[0])
        if n < 1:
            raise ValueError("%s: mask_depth holds no object" % what)
        hm = int(np.shape(depth_heightmap)[-1])
        n_pairs = n * (n - 1) // 2 if is_ets else 0
        idx = val = pair_list = rows = None
        calls, kept = [], {}              # per primitive: (offset into idx / val, groups, maps per group)
        for style, name in ((0, "grasp"), (1, "suction"), (2, "pairs")):
            if style == 2:
                if not n_pairs:
                    break
                model, q, m, pair_list = self._object_pair_maps(depth_heightmap, mask_depth, is_target)
                groups, per = len(pair_list), 1
                rots = [(0, model.gnum_rotations)] * groups
                mask_a, mask_b = [g for g, _ in pair_list], [s_ for _, s_ in pair_list]
            else:
                model, q, m, groups, per = self._object_maps(what, depth_heightmap, mask_depth, style, is_target)
                rots = [(r, per) for k_ in range(groups) for r in range(per)]
                mask_a, mask_b = [k_ for k_ in range(groups) for r in range(per)], [-1] * (groups * per)
            if idx is None and pick is not None:
                idx = torch.empty((2 * n + n_pairs, k), dtype=torch.int32, device=q.device)
                val = torch.empty((2 * n + n_pairs, k), dtype=torch.float32, device=q.device)
            if rows is None and stats is not None:
                rows = torch.empty((len(betas), 2 * n + n_pairs, 4), dtype=torch.float64, device=q.device)
            off = sum(c[1] for c in calls)
            eng, aff, _, stream = self._scene_call(model, q, depth_heightmap, rots)
            group_of = [j // per for j in range(len(rots))]
            if joint:
                groups, group_of = 1, [0] * len(rots)
            if pick is not None:
                pick(eng, q, len(rots), aff, hm, m, mask_a, mask_b, group_of, groups, idx[off:].data_ptr(), val[off:].data_ptr(), stream, style)
            for j, beta in enumerate(betas if stats is not None else ()):
                stats(eng, q, len(rots), aff, hm, m, mask_a, mask_b, group_of, groups, rows[j, off:].data_ptr(), stream, beta)
            calls.append((off, groups, per))
            kept[name] = q
        self._last_object_q = kept        # the maps behind the result, object-major: "grasp" / "suction" [n * R, HEAD_OUT, OH, OW], "pairs" [n_pairs, HEAD_OUT, OH, OW]
        rows = None if rows is None else rows.cpu().numpy()
        if pick is None:
            return calls, None, None, pair_list, hm, rows
        return calls, idx.cpu().numpy(), val.cpu().numpy().astype(np.float64), pair_list, hm, rows

    @staticmethod
    def _scene_entry(i, conf, hm, per):
        """A flattened index into [groups * per, hm, hm] and its value -> (rotation, (iy, ix), conf), or None for index -1."""
        i = int(i)
        return None if i < 0 else ((i // (hm * hm)) % per, ((i // hm) % hm, i % hm), conf)

    def _best_scene_objects(self, what, depth_heightmap, mask_depth, is_ets, is_target, argmax):
        """The body of best_scene_actions and best_scene_class_actions (the caller has checked method and geometry):
        _scene_object_picks with one pair per group, and the host decode of index -> (object, rotation, pixel)."""
        calls, i_all, v_all, pair_list, hm, _ = self._scene_object_picks(what, depth_heightmap, mask_depth, is_ets, is_target, argmax)

        def decode(off, groups, per):
            """Per group (rotation, (iy, ix), conf) or None, and the overall best group or None."""
            entries = [self._scene_entry(i_all[off + k, 0], v_all[off + k, 0], hm, per) for k in range(groups)]
            have = [k for k in range(groups) if entries[k] is not None]
            return entries, (have[int(np.argmax([entries[k][2] for k in have]))] if have else None)
        out = {"per_object": {}}
        for (off, groups, per), name, key in zip(calls, ("grasp", "suction"), ("bestg", "bests")):
            entries, best = decode(off, groups, per)
            out["per_object"][name] = entries
            out[key + "_id"] = None if best is None else (best, entries[best][0])
            out[key + "_pixel"] = None if best is None else entries[best][1]
            out[key + "_conf"] = -np.inf if best is None else entries[best][2]
        out.update(bestgs_num=None, bestgs_pixel=None, bestgs_conf=0)
        if len(calls) == 3:
            entries, best = decode(*calls[2])
            out["bestgs_conf"] = -np.inf
            if best is not None:
                out.update(bestgs_num=pair_list[best], bestgs_pixel=entries[best][1], bestgs_conf=entries[best][2])
        return out

    @staticmethod
    def _require_ranks(what, k, radius):
        if int(k) != k or k < 1 or k > 32:
            raise ValueError("%s: k must be an integer from 1 to 32 (the engine's kSceneTopK)" % what)
        if int(radius) != radius or radius < 0:
            raise ValueError("%s: radius must be an integer >= 0, in heightmap pixels" % what)
        return int(k), int(radius)

    def _ranked_scene_objects(self, what, depth_heightmap, mask_depth, k, is_ets, is_target, topk, joint=False, stats=None, beta=None):
        """The body of ranked_scene_actions, sampled_scene_actions and their class forms (the caller has checked method, geometry
        and the pick's own arguments): _scene_object_picks with k pairs per group and the host decode of every rank (draw).
        `joint` (the sampled forms): one group per primitive, decoded to (object, rotation, pixel, conf) per draw.
        `stats` (the sampled forms' with_stats): the statistics call at `beta` on the same maps; the result gains "stats" and
        "logp" (_with_logp)."""
        calls, i_all, v_all, pair_list, hm, rows = self._scene_object_picks(what, depth_heightmap, mask_depth, is_ets, is_target, topk, k, joint,
                                                                            stats, () if stats is None else (beta,))
        if stats is not None:
            return self._with_logp(self._ranked_decode(calls, i_all, v_all, pair_list, hm, k, joint), calls, rows[0], beta, joint)
        return self._ranked_decode(calls, i_all, v_all, pair_list, hm, k, joint)

    def _ranked_decode(self, calls, i_all, v_all, pair_list, hm, k, joint):
        """_ranked_scene_objects' host decode of what _scene_object_picks read back."""

        def decode(off, groups, per):
            lists = [[self._scene_entry(i_all[off + g, j], v_all[off + g, j], hm, per) for j in range(k)] for g in range(groups)]
            return [[e for e in entries if e is not None] for entries in lists]        # (an exhausted group's -1 tail is dropped)

        def order(lists, item):
            """Every entry of the lists in the order repeated np.argmax takes them: a NaN first, then descending, then (group, rank)."""
            flat = [(g, j, e) for g, entries in enumerate(lists) for j, e in enumerate(entries)]
            flat.sort(key=lambda x: (0, 0.0, x[0], x[1]) if np.isnan(x[2][-1]) else (1, -x[2][-1], x[0], x[1]))       # (the confidence is an entry's last item)
            return [item(g, e) for g, _, e in flat]
        if joint:
            def whole(off, per):
                """The draws of the primitive's one group: (map // per, rotation, (iy, ix), conf), a -1 dropped."""
                drawn = [(int(i_all[off, j]), self._scene_entry(i_all[off, j], v_all[off, j], hm, per)) for j in range(k)]
                return [(i // (hm * hm) // per,) + e for i, e in drawn if e is not None]
            out = {"joint": {"pairs": []}, "pairs": [], "per_pair": [], "ranked": {}}
            for (off, _, per), name in zip(calls, ("grasp", "suction")):
                out["joint"][name] = whole(off, per)
            if len(calls) == 3:
                out["pairs"] = list(pair_list)
                out["joint"]["pairs"] = [(pair_list[g], pixel, conf) for g, _, pixel, conf in whole(calls[2][0], 1)]
            for name, entries in out["joint"].items():
                out["ranked"][name] = order([[e] for e in entries], lambda g, e: e)
            return out
        out = {"per_object": {}, "pairs": [], "per_pair": [], "ranked": {"pairs": []}}
        for call, name in zip(calls, ("grasp", "suction")):
            out["per_object"][name] = decode(*call)
            out["ranked"][name] = order(out["per_object"][name], lambda g, e: (g,) + e)
        if len(calls) == 3:
            out["pairs"], out["per_pair"] = list(pair_list), decode(*calls[2])
            out["ranked"]["pairs"] = order(out["per_pair"], lambda g, e: (pair_list[g], e[1], e[2]))
        return out

    def ranked_scene_actions(self, depth_heightmap, mask_depth, k, radius, is_ets=True, is_target=False):
        """best_scene_actions with up to `k` SEPARATED actions per object instead of one: the fallbacks a control loop tries on the
        same object when the best pose turns out unreachable.  The same forwards - one per primitive, the maps kept in
        self._last_object_q -, one smg_scene_topk_objects per primitive and one read-back.  Rank 0 of an object is
        best_scene_actions' entry; rank j is the best of the object's own pixels (over all its rotations) that lie farther than
        `radius` heightmap pixels from every earlier pick of that object, whichever rotation picked it (radius 0: any other pixel).
        Returns per_object = {"grasp": [...], "suction": [...]}: per object a list of up to k (rotation, (iy, ix), conf) in rank
        order, shorter (or empty) where the object has no pixel left; pairs = [(g, s)] and per_pair, the same lists per pair
        (both [] with fewer than two objects or is_ets False); ranked = {"grasp": [(object, rotation, (iy, ix), conf)], "suction":
        [...], "pairs": [((g, s), (iy, ix), conf)]}: all entries of a primitive by confidence, as repeated np.argmax orders them (a
        NaN first, then descending, the lower (object, rank) on ties).  ranked_to_best turns one of them into the dict that
        get_label_value_scene and backprop_scene read.  1 <= k <= 32 and radius >= 0, else ValueError."""
        self._require_scene("ranked_scene_actions", depth_heightmap)
        k, radius = self._require_ranks("ranked_scene_actions", k, radius)

        def topk(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, idx, val, stream, style):
            eng.scene_topk_objects(q.data_ptr(), q.shape[2] * q.shape[3], n_maps, aff, hm, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                   group_of, groups, k, radius, idx, val, stream)
        return self._ranked_scene_objects("ranked_scene_actions", depth_heightmap, mask_depth, k, is_ets, is_target, topk)

    @staticmethod
    def _require_draws(what, n_draws, temperature, seed):
        """-> (n_draws, beta = 1 / temperature, seed) of the sampled forms, or ValueError."""
        if isinstance(n_draws, bool) or int(n_draws) != n_draws or not 1 <= n_draws <= 32:
            raise ValueError("%s: n_draws must be an integer from 1 to 32 (the engine's kSceneDraws)" % what)
        if not temperature > 0:                            # (a NaN fails this too)
            raise ValueError("%s: temperature must be > 0 (inf draws uniformly)" % what)
        if isinstance(seed, (bool, float)) or int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError("%s: seed must be an integer in [0, 2^64)" % what)
        return int(n_draws), 1.0 / float(temperature), int(seed)

    @staticmethod
    def _style_seed(seed, style):
        """The seed of the sample call for primitive `style`: without the step the primitives would share one noise field."""
        return (seed + style * 0x9E3779B97F4A7C15) % 2 ** 64

    def sampled_scene_actions(self, depth_heightmap, mask_depth, n_draws, temperature, seed, is_ets=True, is_target=False, joint=False,
                              with_stats=False):
        """EXPLORATION for best_scene_actions: instead of the best pixel, `n_draws` independent Boltzmann draws per object - a
        (rotation, pixel) of the object's own pixels drawn with probability proportional to exp(Q / temperature).  The same
        forwards - one per primitive, the maps kept in self._last_object_q -, one smg_scene_sample_objects per primitive and one
        read-back; nothing of [n * R, hm, hm] is written.  temperature = inf draws uniformly over the object's pixels with a
        window, a small temperature approaches best_scene_actions.  The draw is a pure function of (maps, masks, temperature,
        seed): the noise is the counter-based hash include/smg_hip.h states, and primitive s uses the seed
        (seed + s * 0x9E3779B97F4A7C15) mod 2^64.  Draw d does not depend on n_draws.
        Returns ranked_scene_actions' keys: per_object = {"grasp": [...], "suction": [...]}, per object a list of up to n_draws
        (rotation, (iy, ix), conf) in DRAW order (empty where the object has no pixel with a window), conf = the Q value there;
        pairs and per_pair; ranked = all draws of a primitive by confidence.  ranked_to_best serves unchanged, so a sampled action
        that was executed goes through get_label_value_scene and backprop_scene like the best one.
        joint=True: all objects of a primitive form ONE group, the draw is over (object, rotation, pixel) jointly; per_object is
        replaced by joint = {"grasp": [(object, rotation, (iy, ix), conf)], "suction": [...], "pairs": [((g, s), (iy, ix), conf)]}
        in draw order, per_pair is [], and ranked is built from it.
        with_stats=True: one smg_scene_softmax_objects per primitive is enqueued on the same maps and masks before the read-back,
        and two keys are added - stats = scene_policy_stats' dict at this temperature, and logp = {"grasp": [...], "suction":
        [...], "pairs": [...]}, lists parallel to per_object / per_pair (or to joint) with log pi = conf / temperature - lse of the
        entry's group in float64: the behaviour policy's log-probability of every draw.
        1 <= n_draws <= 32, temperature > 0 and 0 <= seed < 2^64, else ValueError."""
        self._require_scene("sampled_scene_actions", depth_heightmap)
        n_draws, beta, seed = self._require_draws("sampled_scene_actions", n_draws, temperature, seed)

        def sample(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, idx, val, stream, style):
            eng.scene_sample_objects(q.data_ptr(), q.shape[2] * q.shape[3], n_maps, aff, hm, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                     group_of, groups, n_draws, beta, self._style_seed(seed, style), idx, val, stream)
        return self._ranked_scene_objects("sampled_scene_actions", depth_heightmap, mask_depth, n_draws, is_ets, is_target, sample, joint,
                                          self._q_softmax if with_stats else None, beta)

    # ---- the normaliser of the Boltzmann policy: log-sum-exp, mean, entropy and mellowmax per object ---------------------------------
    @staticmethod
    def _q_softmax(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, rows, stream, beta):
        eng.scene_softmax_objects(q.data_ptr(), q.shape[2] * q.shape[3], n_maps, aff, hm, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                  group_of, groups, beta, rows, stream)

    @staticmethod
    def _class_softmax(cls):
        def stats(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, rows, stream, beta):
            eng.scene_class_softmax_objects(q.data_ptr(), n_maps, aff, hm, cls, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                            group_of, groups, beta, rows, stream)
        return stats

    @staticmethod
    def _require_betas(what, temperature):
        """-> (betas = 1 / temperature per entry, whether `temperature` was a sequence), validated as _require_draws validates it."""
        seq = not np.isscalar(temperature)
        ts = [float(t) for t in temperature] if seq else [float(temperature)]
        if not ts or not all(t > 0 for t in ts):               # (a NaN fails this too)
            raise ValueError("%s: temperature must be > 0 (inf is the uniform policy)" % what)
        return [1.0 / t for t in ts], seq

    @staticmethod
    def _policy_stats(rows, beta):
        """Rows [..., groups, 4] = {count, vmax, lse, mean} and beta (a scalar, or [temperatures, 1]) -> scene_policy_stats' dict of
        one primitive: entropy = lse - beta mean, mellowmax = (lse - log count) / beta (beta = 0, the uniform policy: the mean)."""
        rows = np.asarray(rows, dtype=np.float64)
        beta = np.asarray(beta, dtype=np.float64)
        count, vmax, lse, mean = (rows[..., c] for c in range(4))
        with np.errstate(invalid="ignore", divide="ignore"):
            soft = np.where(beta > 0, (lse - np.log(count)) / np.where(beta > 0, beta, 1.0), mean)
            return dict(count=count, vmax=vmax, lse=lse, mean=mean, entropy=lse - beta * mean, mellowmax=soft, beta=beta)

    def _policy_stats_out(self, calls, rows, betas, seq):
        """The statistics _scene_object_picks read back ([temperatures, all groups, 4]) as {"grasp", "suction", "pairs"} of
        _policy_stats dicts; a scalar temperature drops the leading axis, "pairs" has no group when no pair was evaluated."""
        beta = np.asarray(betas, dtype=np.float64).reshape(-1, 1) if seq else np.float64(betas[0])
        out = {}
        for j, name in enumerate(("grasp", "suction", "pairs")):
            off, groups = (calls[j][0], calls[j][1]) if j < len(calls) else (0, 0)
            part = rows[:, off:off + groups]
            out[name] = self._policy_stats(part if seq else part[0], beta)
        return out

    def scene_policy_stats(self, depth_heightmap, mask_depth, temperature, is_ets=True, is_target=False, joint=False):
        """What sampled_scene_actions' policy looks like, without drawing from it: per object (per pair) the statistics of the
        Boltzmann policy pi proportional to exp(Q / temperature) over the object's own pixels with a window and all its rotations.
        best_scene_actions' forwards - one per primitive, the maps kept in self._last_object_q -, one smg_scene_softmax_objects per
        primitive and temperature, and one read-back; nothing of [n * R, hm, hm] is written.
        Returns {"grasp": d, "suction": d, "pairs": d}, each d a dict of float64 arrays over the objects (pairs; no entry with
        fewer than two objects or is_ets False): count = the candidates, vmax = the largest Q, lse = log sum exp(Q / temperature)
        - so that log pi(a) = Q(a) / temperature - lse -, mean = the expectation of Q under pi (the expected-SARSA bootstrap),
        entropy = lse - mean / temperature (exp of it = the effective number of candidates), mellowmax = temperature *
        (lse - log count), the soft maximum that lies between the arithmetic mean of Q and `mean` (entropy <= log count); and beta
        = 1 / temperature.  An object without a candidate has
        count 0, vmax and lse -inf and NaN elsewhere.  joint=True: one group per primitive, over (object, rotation, pixel).
        `temperature` may be a sequence: the forwards run once, the maps are reused, and every array gains a leading temperature
        axis.  temperature > 0 (inf: the uniform policy, mellowmax = mean), else ValueError."""
        self._require_scene("scene_policy_stats", depth_heightmap)
        betas, seq = self._require_betas("scene_policy_stats", temperature)
        calls, _, _, _, _, rows = self._scene_object_picks("scene_policy_stats", depth_heightmap, mask_depth, is_ets, is_target, None,
                                                           joint=joint, stats=self._q_softmax, betas=betas)
        return self._policy_stats_out(calls, rows, betas, seq)

    @staticmethod
    def merge_policy_stats(*stats):
        """The merge rule of include/smg_hip.h on the host: the statistics dicts (scene_policy_stats' per primitive, same
        temperature(s)) taken together as ONE candidate set - all groups of all arguments merged in order.  Each group's state is
        recovered as n = count, M = vmax, S = exp(lse - beta M), T = mean S; an empty group is skipped; else M = max (a NaN
        stays), S = SA exp(beta (MA - M)) + SB exp(beta (MB - M)), T likewise, n = nA + nB.  Returns the dict of the merged set,
        its arrays with a last axis of one group: merging the three joint=True primitives gives the policy over all actions,
        merging one primitive's per-object dict gives its joint=True row."""
        if not stats:
            raise ValueError("merge_policy_stats: nothing to merge")
        beta = np.asarray(stats[0]["beta"], dtype=np.float64)
        for d in stats[1:]:
            if not np.array_equal(np.asarray(d["beta"], dtype=np.float64), beta):
                raise ValueError("merge_policy_stats: the statistics were taken at different temperatures")
        b = beta[..., 0] if beta.ndim else beta                # per temperature, without the group axis
        lead = np.shape(stats[0]["count"])[:-1]
        n, M = np.zeros(lead), np.full(lead, -np.inf)
        S, T = np.zeros(lead), np.zeros(lead)
        with np.errstate(invalid="ignore", over="ignore"):
            for d in stats:
                for g in range(np.shape(d["count"])[-1]):
                    nb, Mb = np.asarray(d["count"])[..., g], np.asarray(d["vmax"])[..., g]
                    has = nb > 0
                    Sb = np.where(has, np.exp(np.asarray(d["lse"])[..., g] - np.where(has, b * Mb, 0.0)), 0.0)
                    Tb = np.where(has, np.asarray(d["mean"])[..., g], 0.0) * Sb
                    Mn = np.where((M > Mb) | np.isnan(M), M, Mb)
                    fa, fb = np.exp(b * (M - Mn)), np.exp(b * (Mb - Mn))
                    first = n == 0
                    Sm = np.where(first, Sb, S * np.where(first, 0.0, fa) + Sb * fb)
                    Tm = np.where(first, Tb, T * np.where(first, 0.0, fa) + Tb * fb)
                    S, T = np.where(has, Sm, S), np.where(has, Tm, T)
                    M = np.where(has, np.where(first, Mb, Mn), M)
                    n = n + np.where(has, nb, 0.0)
            some = n > 0
            lse = np.where(some, np.where(some, b * M, 0.0) + np.log(np.where(some, S, 1.0)), -np.inf)
            mean = np.where(some, T / np.where(some, S, 1.0), np.nan)
        rows = np.stack([n, M, lse, mean], axis=-1)[..., None, :]
        return Trainer._policy_stats(rows, beta)

    @staticmethod
    def _with_logp(out, calls, rows, beta, joint):
        """The sampled forms' with_stats: `out` (their decoded dict) gains stats (rows = [all groups, 4] at this beta) and logp =
        beta conf - lse of the entry's group, lists parallel to per_object / per_pair, or to joint."""
        stats, logp = {}, {}
        for j, name in enumerate(("grasp", "suction", "pairs")):
            off, groups = (calls[j][0], calls[j][1]) if j < len(calls) else (0, 0)
            stats[name] = Trainer._policy_stats(rows[off:off + groups], np.float64(beta))
            lse = stats[name]["lse"]
            if joint:
                logp[name] = [beta * np.float64(e[-1]) - lse[0] for e in out["joint"][name]]
            else:
                lists = out["per_pair"] if name == "pairs" else out["per_object"][name]
                logp[name] = [[beta * np.float64(e[-1]) - lse[g] for e in entries] for g, entries in enumerate(lists)]
        out["stats"], out["logp"] = stats, logp
        return out

    @staticmethod
    def ranked_to_best(ranked, primitive_action, j):
        """Entry `j` of ranked_scene_actions' / ranked_scene_class_actions' result (the dict, or its "ranked" part) for the primitive
        'grasp' / 'suction' / 'grasp_then_suction', as a dict with best_scene_actions' keys: the chosen primitive's bestg_id /
        bests_id = (object, rotation) or bestgs_num = (g, s), its _pixel and _conf; the other primitives None / None / -inf (pair:
        0).  A fallback that was executed goes through get_label_value_scene and backprop_scene as the best action would."""
        if primitive_action not in _ACTION_STYLE:
            raise ValueError("ranked_to_best: unknown primitive %r" % (primitive_action,))
        lists = ranked.get("ranked", ranked)
        name = ("grasp", "suction", "pairs")[_ACTION_STYLE[primitive_action]]
        if int(j) != j or not 0 <= j < len(lists[name]):
            raise ValueError("ranked_to_best: no entry %r among the %d ranked %s actions" % (j, len(lists[name]), primitive_action))
        out = dict(bestg_id=None, bestg_pixel=None, bestg_conf=-np.inf, bests_id=None, bests_pixel=None, bests_conf=-np.inf,
                   bestgs_num=None, bestgs_pixel=None, bestgs_conf=0)
        e = lists[name][int(j)]
        if name == "pairs":
            out.update(bestgs_num=tuple(e[0]), bestgs_pixel=tuple(e[1]), bestgs_conf=e[2])
        else:
            key = "bestg" if name == "grasp" else "bests"
            out.update({key + "_id": (e[0], e[1]), key + "_pixel": tuple(e[2]), key + "_conf": e[3]})
        return out

    @staticmethod
    def _scene_pixel_args(pixels, n, hm, labels, weights=None, class_labels=False):
        """What train_batch_scene_pixels and train_batch_scene_class_pixels check of their lists, in this order: `pixels` [n, K, 2]
        ([n, 2] is K = 1); `labels` and, unless None, `weights` [n, K] ([n] for K = 1); with `class_labels`, labels that are class
        indices 0, 1 or 2; integer (iy, ix) inside the hm x hm heightmap.
        Returns the pixels as int64 [n, K, 2], K, and labels and weights as float32 [n, K] (weights None stays None)."""
        pix = np.asarray(pixels)
        if pix.ndim == 2:
            pix = pix[:, None, :]
        if pix.ndim != 3 or pix.shape[0] != n or pix.shape[1] < 1 or pix.shape[2] != 2:
            raise ValueError("pixels must be [%d samples, K, 2] = (iy, ix), got %s" % (n, np.shape(pixels)))
        K = pix.shape[1]
        lab = np.asarray(labels, dtype=np.float32)
        wgt = None if weights is None else np.asarray(weights, dtype=np.float32)
        for name, a in (("labels", lab), ("weights", wgt)):
            if a is not None and a.shape != (n, K) and not (K == 1 and a.shape == (n,)):
                raise ValueError("%s must be [%d samples, %d], got %s" % (name, n, K, a.shape))
        lab, wgt = lab.reshape(n, K), None if wgt is None else wgt.reshape(n, K)
        if class_labels and not np.isin(lab, (0.0, 1.0, 2.0)).all():      # (torch's nll_loss raises on a class index outside [0, 3), as in train_batch)
            raise ValueError("labels must be class indices 0, 1 or 2")
        pix_i = pix.astype(np.int64)
        if not np.array_equal(pix_i, pix) or pix_i.min() < 0 or pix_i.max() >= hm:
            raise ValueError("pixels must be integer (iy, ix) inside the %d x %d heightmap" % (hm, hm))
        return pix_i, K, lab, wgt

    @staticmethod
    def _scene_affines(rots, num):
        import models
        return [models.rotation_theta(r, num) for r in rots]

    def train_batch_scene_pixels(self, depth_heightmap, m_depth_heightmap, style, rotations, pixels, labels, weights=None, grad_sync=None,
                                 return_q=False):
        """train_batch_maps with the labels at HEIGHTMAP pixels: sample j trains K scene pixels - `pixels` [n_samples, K, 2] =
        (iy, ix) ([n_samples, 2] for K = 1), `labels` / `weights` [n_samples, K] (weights None = all ones) - through the bilinear
        interpolation of its Q map at those points: loss_j = sum_k w * Huber(v_k - label_k) (smg_loss_scene), whose gradient
        spreads over the four map elements around each point.  A pixel without a window of the head in its sample's rotation
        (scene_to_map's `valid`) raises ValueError before anything runs.  The gradient of the SUM of the losses goes back in one
        backward pass (dense head form), then ONE Adam step.  Scenes, rotations and `grad_sync` as in train_batch_maps; host
        arrays.  Reinforcement method only.  Returns the loss vector (and q [n_samples, 1, OH, OW] if asked)."""
        _, _, side = self._require_scene("train_batch_scene_pixels", depth_heightmap)
        rots = self._flat_rotations(depth_heightmap, style, rotations)
        n, num, hm = len(rots), self.model.gnum_rotations, int(np.shape(depth_heightmap)[-1])
        pix_i, K, lab, wgt = self._scene_pixel_args(pixels, n, hm, labels, weights)
        _, _, valid = self.scene_to_map(hm, np.asarray(rots).reshape(n, 1), num, pix_i)
        if not valid.all():
            j, k = np.argwhere(~valid)[0]
            raise ValueError("pixel %s of sample %d has no Q window in rotation %d of %d (scene_to_map)" % (tuple(pix_i[j, k]), j, rots[j], num))

        def loss_call(eng, q, tensors, n, loss, dq, stream):
            eng.loss_scene(q.data_ptr(), self._scene_affines(rots, num), hm, n, K, _ptr(tensors[0]), _ptr(tensors[1]), _ptr(tensors[2]),
                           loss.data_ptr(), dq.data_ptr(), stream)
        return self._train_maps(depth_heightmap, m_depth_heightmap, style, rotations, (1, side),
                                lambda dev: (_i32_on(dev, pix_i), _f32_on(dev, lab), _f32_on(dev, wgt)), loss_call, grad_sync, return_q)

    def train_batch_scene_maps(self, depth_heightmap, m_depth_heightmap, style, rotations, label_maps, weight_maps=None, grad_sync=None,
                               return_q=False):
        """train_batch_scene_pixels with a whole label IMAGE per sample: `label_maps` / `weight_maps` are host arrays
        [n_samples, hm, hm] in heightmap pixels, scene-major (`weight_maps` None = all ones, a weight of 0 masks its pixel, the label
        under it may be anything).  loss_j = sum over the pixels that have a window of the head in sample j's rotation
        (scene_to_map's `valid`) of w * Huber(v - label), v the bilinear interpolation of the sample's Q map there
        (smg_loss_scene_map).  Pixels without a window contribute nothing and raise nothing: a whole image always covers such
        pixels.  The gradient of the SUM of the losses goes back in one backward pass (dense head form), then ONE Adam step.
        Scenes, rotations and `grad_sync` as in train_batch_scene_pixels.  Reinforcement method only.  Returns the loss vector
        (and q [n_samples, 1, OH, OW] if asked)."""
        _, _, side = self._require_scene("train_batch_scene_maps", depth_heightmap)
        rots = self._flat_rotations(depth_heightmap, style, rotations)
        n, num, hm = len(rots), self.model.gnum_rotations, int(np.shape(depth_heightmap)[-1])
        for name, maps in (("label_maps", label_maps), ("weight_maps", weight_maps)):
            if (maps is not None or name == "label_maps") and (maps is None or tuple(np.shape(maps)) != (n, hm, hm)):
                raise ValueError("%s must be [%d samples, %d, %d] for a %d^2 heightmap, got %s"
                                 % (name, n, hm, hm, hm, None if maps is None else tuple(np.shape(maps))))

        def loss_call(eng, q, tensors, n, loss, dq, stream):
            eng.loss_scene_map(q.data_ptr(), self._scene_affines(rots, num), hm, n, _ptr(tensors[0]), _ptr(tensors[1]),
                               loss.data_ptr(), dq.data_ptr(), stream)
        return self._train_maps(depth_heightmap, m_depth_heightmap, style, rotations, (1, side),
                                lambda dev: (_f32_on(dev, label_maps), _f32_on(dev, weight_maps)), loss_call, grad_sync, return_q)

    def train_batch_scene_policy(self, depth_heightmap, m_depth_heightmap, style, rotations, select_masks, sample_masks, sample_groups, actions,
                                 temperature, nll_weights=None, entropy_weights=None, grad_sync=None, return_q=False, return_stats=False):
        """TRAIN the Boltzmann policy sampled_scene_actions explores with: the samples (scene, rotation) form groups, the policy
        of a group is pi proportional to exp(Q / temperature) over the selected pixels with a window of all its samples, and the
        loss of group g is  w_nll (lse - v_act / temperature) - w_ent H  (smg_loss_scene_policy): the negative log-likelihood of the
        executed action - w_nll 1 clones a demonstration, an advantage makes it the policy-gradient step, it may be negative - and
        the entropy H = lse - mean / temperature as a bonus.  `select_masks` [n_masks, hm, hm] (a pixel is selected where its mask
        is not exactly 0); `sample_masks[j]` = the mask index of sample j, a pair of indices (their union) or -1 (every pixel);
        `sample_groups[j]` = its group in [0, n_groups), n_groups = len(actions); `actions[g]` = None or (sample j, (iy, ix));
        `nll_weights` / `entropy_weights` [n_groups], None = all ones / all zeros.  One forward, ONE loss call, one backward
        (dense head form), ONE Adam step (_train_maps).  ValueError before anything runs for: an action whose sample is not in
        its group, a pixel outside the heightmap, without a window in that sample's rotation (scene_to_map) or not selected by the
        sample's masks, a temperature that is no positive scalar, weights that are not finite.  Reinforcement method only.
        Returns the loss [n_groups] (then q [n_samples, 1, OH, OW] and / or the float64 rows [n_groups, 4] = {count, vmax, lse,
        mean} of smg_scene_softmax_objects if asked), device tensors."""
        what = "train_batch_scene_policy"
        _, _, side = self._require_scene(what, depth_heightmap)
        rots = self._flat_rotations(depth_heightmap, style, rotations)
        n, num, hm = len(rots), self.model.gnum_rotations, int(np.shape(depth_heightmap)[-1])
        if not np.isscalar(temperature) or not float(temperature) > 0:                 # (a NaN fails this too)
            raise ValueError("%s: temperature must be one number > 0 (inf is the uniform policy)" % what)
        beta = 1.0 / float(temperature)
        masks = np.ascontiguousarray(select_masks, dtype=np.float64)
        if masks.ndim != 3 or masks.shape[0] < 1 or masks.shape[1:] != (hm, hm):
            raise ValueError("%s: select_masks must be [n_masks >= 1, %d, %d], got %s" % (what, hm, hm, masks.shape))
        if len(sample_masks) != n or len(sample_groups) != n:
            raise ValueError("%s: one sample_masks entry and one sample_groups entry per sample (%d)" % (what, n))
        mask_a, mask_b = [], []
        for sm in sample_masks:
            a, b = (int(sm), -1) if np.isscalar(sm) else (int(sm[0]), int(sm[1])) if len(sm) == 2 else (None, None)
            if a is None or not (-1 <= a < masks.shape[0] and -1 <= b < masks.shape[0]):
                raise ValueError("%s: sample_masks entries are a mask index, a pair of indices or -1, inside [-1, %d)" % (what, masks.shape[0]))
            mask_a.append(a)
            mask_b.append(b)
        n_groups = len(actions)
        groups = [int(g) for g in sample_groups]
        if n_groups < 1 or not all(0 <= g < n_groups for g in groups):
            raise ValueError("%s: sample_groups must lie in [0, len(actions) = %d)" % (what, n_groups))
        wgt = np.empty((n_groups, 2), dtype=np.float64)
        for c, (name, w, default) in enumerate((("nll_weights", nll_weights, 1.0), ("entropy_weights", entropy_weights, 0.0))):
            w = np.full(n_groups, default) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
            if w.shape != (n_groups,) or not np.isfinite(w).all():
                raise ValueError("%s: %s must be %d finite numbers" % (what, name, n_groups))
            wgt[:, c] = w
        if n * hm * hm > 0x7fffffff:
            raise ValueError("%s: the flattened action index does not fit int32" % what)
        act = np.full(n_groups, -1, dtype=np.int32)
        for g, a in enumerate(actions):
            if a is None:
                continue
            j, (iy, ix) = a
            if int(j) != j or not 0 <= j < n or groups[int(j)] != g:
                raise ValueError("%s: the action of group %d names sample %r, which is not in that group" % (what, g, j))
            j = int(j)
            if int(iy) != iy or int(ix) != ix or not (0 <= iy < hm and 0 <= ix < hm):
                raise ValueError("%s: the action pixel %r of group %d lies outside the %d x %d heightmap" % (what, (iy, ix), g, hm, hm))
            iy, ix = int(iy), int(ix)
            if not self.scene_to_map(hm, rots[j], num, [[iy, ix]])[2][0]:
                raise ValueError("%s: the action pixel %r of group %d has no Q window in rotation %d of %d (scene_to_map)" % (what, (iy, ix), g, rots[j], num))
            if (mask_a[j] >= 0 or mask_b[j] >= 0) and not any(t >= 0 and masks[t, iy, ix] != 0 for t in (mask_a[j], mask_b[j])):
                raise ValueError("%s: the action pixel %r of group %d is not selected by the masks of sample %d" % (what, (iy, ix), g, j))
            act[g] = (j * hm + iy) * hm + ix
        kept = {}

        def loss_call(eng, q, tensors, n, loss, dq, stream):
            kept["stats"] = torch.empty((n_groups, 4), dtype=torch.float64, device=q.device)
            eng.loss_scene_policy(q.data_ptr(), self._scene_affines(rots, num), hm, n, tensors[0].data_ptr(), int(masks.shape[0]), mask_a, mask_b,
                                  groups, n_groups, beta, tensors[1].data_ptr(), tensors[2].data_ptr(), kept["stats"].data_ptr(),
                                  loss.data_ptr(), dq.data_ptr(), stream)
        out = self._train_maps(depth_heightmap, m_depth_heightmap, style, rotations, (1, side),
                               lambda dev: (torch.as_tensor(masks, device=dev), _i32_on(dev, act), torch.as_tensor(wgt, device=dev)),
                               loss_call, grad_sync, return_q, n_loss=n_groups)
        if not return_stats:
            return out
        return (out + (kept["stats"],)) if return_q else (out, kept["stats"])

    # ---- dense class maps (reactive method on heightmaps larger than 224^2: three logits per 20x20 window of the feature plane) ---
    def _require_reactive(self, what):
        if self.method != 'reactive':
            raise ValueError("%s: reactive method only (three class logits per pixel; the reinforcement head's maps are "
                             "forward_dense / train_batch_maps)" % what)

    def forward_class_maps(self, depth_heightmap, m_depth_heightmap, style=0, specific_rotation=-1, logits=False, return_device=False):
        """The reactive Trainer.forward(..., is_volatile=True) without the one-pixel restriction: the class probabilities of every
        evaluated rotation, float64 [R, 3, OH, OW] (softmax over axis 1 on the device, as forward's; `logits` = the raw head
        output instead) - or the float32 device tensor of that shape if asked.  Rotation choice and BN bookkeeping are forward's;
        a 224^2 heightmap gives [R, 3, 1, 1] whose element [0, 0, 0, 0] is forward's P(success).  Reactive method only."""
        self._require_reactive("forward_class_maps")
        with np.errstate(divide="ignore", invalid="ignore"):
            q = self._evaluate(self.model, depth_heightmap, m_depth_heightmap, style, True, specific_rotation)
        self._last_q = q
        p = q if logits else torch.softmax(q, dim=1)
        return p if return_device else p.cpu().numpy().astype(np.float64)

    def best_class_map_action(self, depth_heightmap, m_depth_heightmap, style=0):
        """The (rotation, pixel) of the sweep with the largest P(class 0), found on the device (smg_argmax over the flattened
        [R, OH, OW]: lowest index on ties like np.argmax); the host reads back one (index, value) pair.
        Returns {"rotation", "pixel": (oy, ox), "conf"}."""
        p = self.forward_class_maps(depth_heightmap, m_depth_heightmap, style, return_device=True)
        p0 = p[:, 0].contiguous()
        dev = p0.device
        idx = torch.empty(1, dtype=torch.int32, device=dev)
        val = torch.empty(1, dtype=torch.float32, device=dev)
        smg_hip.argmax(p0.data_ptr(), p0.numel(), idx.data_ptr(), val.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        i = int(idx.cpu().numpy()[0])
        _, OH, OW = p0.shape
        return {"rotation": i // (OH * OW), "pixel": ((i // OW) % OH, i % OW), "conf": float(val.cpu().numpy().astype(np.float64)[0])}

    def train_batch_class_maps(self, depth_heightmap, m_depth_heightmap, style, rotations, label_maps, grad_sync=None, return_q=False):
        """train_batch with a whole map of class labels per sample - the reference's own criterion (CrossEntropyLoss2d,
        code/utils.py:306-313, class weights {1, 1, 0}) on the whole head output: the loss of sample j is the mean over its
        labelled pixels (classes 0 / 1) of the cross entropy, class 2 masks a pixel ("no loss", code/trainer.py:38-60); a map
        without a labelled pixel gives loss 0 and no gradient (smg_loss_map_ce).  The gradient of the SUM of the losses goes back
        in one backward pass, then ONE Adam step.  Scenes, rotations, host or device inputs and `grad_sync` as in
        train_batch_maps; `label_maps` is [n_samples, OH, OW] (dense_map_size), scene-major; host arrays are checked for values
        outside {0, 1, 2}, device tensors are not read back.  Reactive method only.
        Returns the loss vector (and the logits q [n_samples, 3, OH, OW] if asked)."""
        self._require_reactive("train_batch_class_maps")
        n = len(self._flat_rotations(depth_heightmap, style, rotations))
        side = self.dense_map_size(np.shape(depth_heightmap)[-1])
        if tuple(label_maps.shape if torch.is_tensor(label_maps) else np.shape(label_maps)) != (n, side, side):
            raise ValueError("label_maps must be [%d samples, %d, %d] for a %d^2 heightmap, got %s"
                             % (n, side, side, np.shape(depth_heightmap)[-1], tuple(np.shape(label_maps))))
        if not torch.is_tensor(label_maps):
            label_maps = np.ascontiguousarray(label_maps, dtype=np.float32)
            if not np.isin(label_maps, (0.0, 1.0, 2.0)).all():      # (torch's nll_loss raises on a class index outside [0, 3), as in train_batch)
                raise ValueError("label maps must hold class indices 0, 1 or 2")

        def loss_call(eng, q, lab, n, loss, dq, stream):
            eng.loss_map_ce(q.data_ptr(), lab.data_ptr(), n, loss.data_ptr(), dq.data_ptr(), stream)
        return self._train_maps(depth_heightmap, m_depth_heightmap, style, rotations, (3, side),
                                lambda dev: _f32_on(dev, label_maps), loss_call, grad_sync, return_q)

    def train_batch_class_pixels(self, depth_heightmap, m_depth_heightmap, style, rotations, pixels, labels, grad_sync=None, return_q=False):
        """train_batch_class_maps with ONE labelled pixel per sample: `pixels` holds an (oy, ox) per sample, `labels` its class -
        a label map of class 2 ("no loss") everywhere else.  On a 224^2 heightmap pixel (0, 0) is the element train_batch trains."""
        lab = np.asarray(labels, dtype=np.float32).reshape(-1)
        pix = np.asarray(pixels, dtype=np.int64).reshape(-1, 2)
        side = self.dense_map_size(np.shape(depth_heightmap)[-1])
        if len(pix) != len(lab):
            raise ValueError("one (oy, ox) and one label per sample")
        if len(pix) and (pix.min() < 0 or pix.max() >= side):
            raise ValueError("pixels must lie inside the %d x %d class map" % (side, side))
        label_maps = np.full((len(lab), side, side), 2.0, dtype=np.float32)
        label_maps[np.arange(len(lab)), pix[:, 0], pix[:, 1]] = lab
        return self.train_batch_class_maps(depth_heightmap, m_depth_heightmap, style, rotations, label_maps, grad_sync, return_q)

    # ---- class maps in the scene frame (reactive method): logits rotated back and interpolated, softmax at the heightmap pixel ----------
    def _require_scene_class(self, what, depth_heightmap):
        self._require_reactive(what)
        return self._scene_geometry(np.shape(depth_heightmap)[-1])

    def forward_scene_class_maps(self, depth_heightmap, m_depth_heightmap, style=0, specific_rotation=-1, cls=None, logits=False,
                                 return_device=False):
        """forward_class_maps in the SCENE frame: every evaluated rotation's three logit maps rotated back and bilinearly
        interpolated at the heightmap's pixels, softmax taken there (smg_scene_class_maps) - float64 [R, 3, hm, hm] class
        probabilities, or [R, hm, hm] for one `cls` in {0, 1, 2}; the float32 device tensor if asked; -inf where no window of the
        head is centred in that rotation.  `logits` returns the interpolated logits instead (smg_scene_maps per class plane).
        Element [r, c, iy, ix] is P(class c) of acting at heightmap pixel (iy, ix) with rotation r: the same scene point in every
        rotation.  Rotation choice and BN bookkeeping are forward_class_maps'.  Reactive method, heightmaps larger than 224^2."""
        self._require_scene_class("forward_scene_class_maps", depth_heightmap)
        if cls is not None and cls not in (0, 1, 2):
            raise ValueError("forward_scene_class_maps: cls must be None (all three), 0, 1 or 2")
        q = self.forward_class_maps(depth_heightmap, m_depth_heightmap, style, specific_rotation, logits=True, return_device=True)
        dev = q.device
        R, _, OH, OW = q.shape
        eng, aff, hm, stream = self._scene_call(self.model, q, depth_heightmap, self._scene_rotations(self.model, style, specific_rotation))
        if logits:
            planes = (0, 1, 2) if cls is None else (cls,)
            out = torch.empty((len(planes), R, hm, hm), dtype=torch.float32, device=dev)
            for k, c in enumerate(planes):
                eng.scene_maps(q[:, c].data_ptr(), 3 * OH * OW, R, aff, hm, out[k].data_ptr(), stream)
            out = out.permute(1, 0, 2, 3).contiguous() if cls is None else out[0]
        else:
            out = torch.empty((R, 3, hm, hm) if cls is None else (R, hm, hm), dtype=torch.float32, device=dev)
            eng.scene_class_maps(q.data_ptr(), R, aff, hm, -1 if cls is None else cls, out.data_ptr(), stream)
        return out if return_device else out.cpu().numpy().astype(np.float64)

    def best_scene_class_action(self, depth_heightmap, m_depth_heightmap, style=0):
        """The (rotation, heightmap pixel) of the sweep with the largest P(class 0), found on the device without materialising the
        scene-frame maps (smg_scene_class_argmax: lowest index of the flattened [R, hm, hm] on ties like np.argmax, a NaN wins,
        pixels without a window are never picked); the host reads back one (index, value) pair.
        Returns {"rotation", "pixel": (iy, ix), "conf", "map_pixel": (qy, qx)} as best_scene_action does."""
        self._require_scene_class("best_scene_class_action", depth_heightmap)
        q = self.forward_class_maps(depth_heightmap, m_depth_heightmap, style, logits=True, return_device=True)
        rots = self._scene_rotations(self.model, style, -1)
        eng, aff, hm, stream = self._scene_call(self.model, q, depth_heightmap, rots)
        return self._best_scene(q, hm, rots, lambda idx, val: eng.scene_class_argmax(q.data_ptr(), q.shape[0], aff, hm, 0, idx, val, stream))

    # ---- the reactive net per object: the loops of code/main.py:158-195, which run for both methods --------------------------------
    def _require_class_objects(self, what, depth_heightmap, mask_depth):
        """Reactive method, masks [n_objects >= 1, H, H] like the heightmap: checked before anything reaches an engine."""
        self._require_reactive(what)
        shape = tuple(np.shape(mask_depth))
        if len(shape) != 3 or shape[1:] != tuple(np.shape(depth_heightmap)) or shape[1] != shape[2]:
            raise ValueError("%s: mask_depth must be [n_objects, H, H] like the square heightmap, got %s" % (what, shape))
        if shape[0] < 1:
            raise ValueError("%s: mask_depth holds no object" % what)

    def _class_maps_out(self, q, logits, return_device):
        p = q if logits else torch.softmax(q, dim=-3)
        return p if return_device else p.cpu().numpy().astype(np.float64)

    def forward_class_objects(self, depth_heightmap, mask_depth, style=0, logits=False, return_device=False):
        """forward_objects for the reactive net, on any heightmap from 224^2 up - the loop of code/main.py:158-166 with
        forward_class_maps(depth, depth * mask_depth[k], style) in place of the scalar forward: ONE engine call, R + n trunk
        passes, the products formed on the device, BN running statistics updated in the order and count of the reference's loop.
        Returns float64 [n_objects, R, 3, OH, OW] class probabilities (softmax over the class axis on the device, as
        forward_class_maps'; `logits` = the raw head output instead), or the float32 device tensor of that shape if asked.  The
        maps are in the rotated frame of their rotation; OH = OW = 1 at 224^2, where [k, r, 0, 0, 0] is the reactive
        Trainer.forward's P(success).  Styles 0 / 1, reactive method only."""
        self._require_class_objects("forward_class_objects", depth_heightmap, mask_depth)
        _, q, _, n, R = self._object_maps("forward_class_objects", depth_heightmap, mask_depth, style, False)
        return self._class_maps_out(q.reshape(n, R, 3, q.shape[2], q.shape[3]), logits, return_device)

    def forward_class_object_pairs(self, depth_heightmap, mask_depth, logits=False, return_device=False):
        """forward_object_pairs for the reactive net (code/main.py:183-192): style 2, rotation 0, the mask of pair (g < s) is
        mask[g] + mask[s], one engine call with the reference's BN sequence.  Returns (float64 [n_pairs, 3, OH, OW] class
        probabilities - `logits` = the raw head output; the float32 device tensor if asked -, [(g, s)]); with fewer than two objects
        nothing runs and the maps are [0, 3, OH, OW].  Reactive method only."""
        self._require_class_objects("forward_class_object_pairs", depth_heightmap, mask_depth)
        model, q, _, idx = self._object_pair_maps(depth_heightmap, mask_depth, False)
        if q is None:
            side = self.dense_map_size(np.shape(depth_heightmap)[-1])
            q = torch.empty((0, 3, side, side), dtype=torch.float32, device=model._flat_params.device if return_device else "cpu")
        return self._class_maps_out(q, logits, return_device), idx

    def best_scene_class_actions(self, depth_heightmap, mask_depth, is_ets=True, cls=0):
        """best_scene_actions for the reactive net, for a heightmap larger than 224^2: the per-step evaluation of
        code/main.py:158-195 - which the reference runs for both methods - with every object's three logit maps rotated back onto
        the heightmap, the softmax taken at the pixel, and P(class `cls`) read on that object's OWN pixels (mask_depth[k] != 0; for a
        pair (g, s) the pixels of either object).  One engine forward per primitive and one smg_scene_class_argmax_objects on the
        logits and the masks tensor that forward used; neither the n * R scene-frame maps nor masked copies are written, an
        unselected pixel costs no exponential, and the host reads back one (index, value) pair per object and primitive.
        Returns best_scene_actions' dict with its conventions: bestg_id / bests_id = (object, rotation), bestg_pixel / bests_pixel
        = (iy, ix), bestg_conf / bests_conf = P(class cls) there - None, None and -inf when no object has a selected pixel with a
        window -; bestgs_num = (g, s), bestgs_pixel, bestgs_conf (None / None / 0 with fewer than two objects or is_ets False);
        per_object = {"grasp": [...], "suction": [...]}, one (rotation, (iy, ix), conf) per object or None.  The logits behind the
        result stay in self._last_object_q.  There is no is_target: the reactive method has no target net.
        Which primitive to execute is the caller's business: code/main.py:221-226 compares bestg_conf, bests_conf and
        2 * bestgs_conf (the pair's confidence counts twice, for both methods) and takes the largest."""
        self._require_class_objects("best_scene_class_actions", depth_heightmap, mask_depth)
        if cls not in (0, 1, 2):
            raise ValueError("best_scene_class_actions: cls must be 0, 1 or 2")
        self._scene_geometry(np.shape(depth_heightmap)[-1])

        def argmax(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, idx, val, stream, style):
            eng.scene_class_argmax_objects(q.data_ptr(), n_maps, aff, hm, cls, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                           group_of, groups, idx, val, stream)
        return self._best_scene_objects("best_scene_class_actions", depth_heightmap, mask_depth, is_ets, False, argmax)

    def ranked_scene_class_actions(self, depth_heightmap, mask_depth, k, radius, is_ets=True, cls=0):
        """ranked_scene_actions for the reactive net: best_scene_class_actions' forwards, one smg_scene_class_topk_objects per
        primitive on the logits and one read-back - up to `k` pixels per object (per pair) by P(class `cls`), each farther than
        `radius` heightmap pixels from the earlier picks of its object.  Returns ranked_scene_actions' dict (per_object, pairs,
        per_pair, ranked); rank 0 of every list is best_scene_class_actions' entry.  Reactive method only; 1 <= k <= 32,
        radius >= 0 and cls in {0, 1, 2}, else ValueError."""
        self._require_class_objects("ranked_scene_class_actions", depth_heightmap, mask_depth)
        if cls not in (0, 1, 2):
            raise ValueError("ranked_scene_class_actions: cls must be 0, 1 or 2")
        self._scene_geometry(np.shape(depth_heightmap)[-1])
        k, radius = self._require_ranks("ranked_scene_class_actions", k, radius)

        def topk(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, idx, val, stream, style):
            eng.scene_class_topk_objects(q.data_ptr(), n_maps, aff, hm, cls, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                         group_of, groups, k, radius, idx, val, stream)
        return self._ranked_scene_objects("ranked_scene_class_actions", depth_heightmap, mask_depth, k, is_ets, False, topk)

    def sampled_scene_class_actions(self, depth_heightmap, mask_depth, n_draws, temperature, seed, is_ets=True, joint=False, cls=0,
                                    with_stats=False):
        """sampled_scene_actions for the reactive net: best_scene_class_actions' forwards, one smg_scene_class_sample_objects per
        primitive on the logits and one read-back - `n_draws` draws per object (per pair, or with `joint` per primitive) with
        probability proportional to exp(P(class `cls`) / temperature).  Returns sampled_scene_actions' dict; with_stats adds its
        stats and logp keys (one smg_scene_class_softmax_objects per primitive before the read-back).  Reactive method only,
        no is_target; 1 <= n_draws <= 32, temperature > 0, 0 <= seed < 2^64 and cls in {0, 1, 2}, else ValueError."""
        self._require_class_objects("sampled_scene_class_actions", depth_heightmap, mask_depth)
        if cls not in (0, 1, 2):
            raise ValueError("sampled_scene_class_actions: cls must be 0, 1 or 2")
        self._scene_geometry(np.shape(depth_heightmap)[-1])
        n_draws, beta, seed = self._require_draws("sampled_scene_class_actions", n_draws, temperature, seed)

        def sample(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, idx, val, stream, style):
            eng.scene_class_sample_objects(q.data_ptr(), n_maps, aff, hm, cls, m.data_ptr(), int(m.shape[0]), mask_a, mask_b,
                                           group_of, groups, n_draws, beta, self._style_seed(seed, style), idx, val, stream)
        return self._ranked_scene_objects("sampled_scene_class_actions", depth_heightmap, mask_depth, n_draws, is_ets, False, sample, joint,
                                          self._class_softmax(cls) if with_stats else None, beta)

    def scene_class_policy_stats(self, depth_heightmap, mask_depth, temperature, is_ets=True, joint=False, cls=0):
        """scene_policy_stats for the reactive net: best_scene_class_actions' forwards, one smg_scene_class_softmax_objects per
        primitive and temperature on the logits and one read-back - the statistics of the policy proportional to
        exp(P(class `cls`) / temperature) per object (per pair, or with `joint` per primitive).  Returns scene_policy_stats' dict.
        Reactive method only, no is_target; temperature > 0 and cls in {0, 1, 2}, else ValueError."""
        self._require_class_objects("scene_class_policy_stats", depth_heightmap, mask_depth)
        if cls not in (0, 1, 2):
            raise ValueError("scene_class_policy_stats: cls must be 0, 1 or 2")
        self._scene_geometry(np.shape(depth_heightmap)[-1])
        betas, seq = self._require_betas("scene_class_policy_stats", temperature)
        calls, _, _, _, _, rows = self._scene_object_picks("scene_class_policy_stats", depth_heightmap, mask_depth, is_ets, False, None,
                                                           joint=joint, stats=self._class_softmax(cls), betas=betas)
        return self._policy_stats_out(calls, rows, betas, seq)

    def train_batch_scene_class_pixels(self, depth_heightmap, m_depth_heightmap, style, rotations, pixels, labels, grad_sync=None,
                                       return_q=False):
        """train_batch_class_maps with the class labels at HEIGHTMAP pixels: sample j trains K scene pixels - `pixels`
        [n_samples, K, 2] = (iy, ix) ([n_samples, 2] for K = 1), `labels` [n_samples, K] in {0, 1, 2} - through the bilinear
        interpolation of its three logit maps at those points: loss_j = the mean over its class-0 / 1 points of the cross entropy
        of the interpolated logits (smg_loss_scene_ce), whose gradient spreads over the four map elements around each point.
        Class 2 is "no loss": padding for a ragged K, which must lie in the heightmap but needs no window.  A class-0 / 1 pixel
        without a window of the head in its sample's rotation (scene_to_map's `valid`) raises ValueError before anything runs.
        The gradient of the SUM of the losses goes back in one backward pass (dense head form), then ONE Adam step.  Scenes,
        rotations and `grad_sync` as in train_batch_class_maps; host arrays.  Reactive method only.
        Returns the loss vector (and the logits q [n_samples, 3, OH, OW] if asked)."""
        _, _, side = self._require_scene_class("train_batch_scene_class_pixels", depth_heightmap)
        rots = self._flat_rotations(depth_heightmap, style, rotations)
        n, num, hm = len(rots), self.model.gnum_rotations, int(np.shape(depth_heightmap)[-1])
        pix_i, K, lab, _ = self._scene_pixel_args(pixels, n, hm, labels, class_labels=True)
        _, _, valid = self.scene_to_map(hm, np.asarray(rots).reshape(n, 1), num, pix_i)
        lost = ~valid & (lab != 2.0)
        if lost.any():
            j, k = np.argwhere(lost)[0]
            raise ValueError("pixel %s of sample %d (class %d) has no window in rotation %d of %d (scene_to_map)"
                             % (tuple(pix_i[j, k]), j, int(lab[j, k]), rots[j], num))

        def loss_call(eng, q, tensors, n, loss, dq, stream):
            eng.loss_scene_ce(q.data_ptr(), self._scene_affines(rots, num), hm, n, K, _ptr(tensors[0]), _ptr(tensors[1]),
                              loss.data_ptr(), dq.data_ptr(), stream)
        return self._train_maps(depth_heightmap, m_depth_heightmap, style, rotations, (3, side),
                                lambda dev: (_i32_on(dev, pix_i), _f32_on(dev, lab)), loss_call, grad_sync, return_q)

    def train_batch_scene_class_maps(self, depth_heightmap, m_depth_heightmap, style, rotations, label_maps, grad_sync=None,
                                     return_q=False):
        """train_batch_scene_class_pixels with a whole class-label IMAGE per sample: `label_maps` is a host array [n_samples, hm, hm]
        in heightmap pixels, scene-major, of class indices 0, 1 or 2 (anything else, NaN included, raises ValueError as in
        train_batch_class_maps).  loss_j = the mean over the class-0 / 1 pixels that have a window of the head in sample j's
        rotation (scene_to_map's `valid`) of the cross entropy of the interpolated logits (smg_loss_scene_map_ce); class 2 is "no
        loss".  A class-0 / 1 pixel WITHOUT a window is skipped silently - a whole image always covers such pixels - where
        train_batch_scene_class_pixels raises; a sample without a counted pixel gives loss 0 and no gradient.  The gradient of
        the SUM of the losses goes back in one backward pass (dense head form), then ONE Adam step.  Scenes, rotations and
        `grad_sync` as in train_batch_scene_class_pixels.  Reactive method only.
        Returns the loss vector (and the logits q [n_samples, 3, OH, OW] if asked)."""
        _, _, side = self._require_scene_class("train_batch_scene_class_maps", depth_heightmap)
        rots = self._flat_rotations(depth_heightmap, style, rotations)
        n, num, hm = len(rots), self.model.gnum_rotations, int(np.shape(depth_heightmap)[-1])
        if label_maps is None or tuple(np.shape(label_maps)) != (n, hm, hm):
            raise ValueError("label_maps must be [%d samples, %d, %d] for a %d^2 heightmap, got %s"
                             % (n, hm, hm, hm, None if label_maps is None else tuple(np.shape(label_maps))))
        lab_h = np.ascontiguousarray(label_maps, dtype=np.float32)
        if not np.isin(lab_h, (0.0, 1.0, 2.0)).all():      # (torch's nll_loss raises on a class index outside [0, 3), as in train_batch)
            raise ValueError("label maps must hold class indices 0, 1 or 2")

        def loss_call(eng, q, lab, n, loss, dq, stream):
            eng.loss_scene_map_ce(q.data_ptr(), self._scene_affines(rots, num), hm, n, lab.data_ptr(), loss.data_ptr(), dq.data_ptr(), stream)
        return self._train_maps(depth_heightmap, m_depth_heightmap, style, rotations, (3, side),
                                lambda dev: _f32_on(dev, lab_h), loss_call, grad_sync, return_q)

    # ---- the value of a GIVEN action in the scene frame: maps read at listed heightmap pixels (smg_scene_values) -------------------
    @staticmethod
    def _scene_value_pixels(pixels, n, hm):
        """The pixel lists of the scene_*_values methods as int64 [n, K, 2], and whether the caller gave the K axis.  n None: one
        list for every map, [K, 2] or one (iy, ix), returned as [1, K, 2]; else [n, K, 2], or [n, 2] for K = 1.  Integer (iy, ix)
        inside the hm x hm heightmap, as _scene_pixel_args asks; ValueError otherwise."""
        pix = np.asarray(pixels)
        if n is None:
            listed, n, want = True, 1, "[K, 2] or one (iy, ix)"
            pix = pix[None, None] if pix.ndim == 1 else pix[None]
        else:
            listed, want = pix.ndim != 2, "[%d, K, 2] or [%d, 2]" % (n, n)
            if pix.ndim == 2:
                pix = pix[:, None, :]
        if pix.ndim != 3 or pix.shape[0] != n or pix.shape[1] < 1 or pix.shape[2] != 2:
            raise ValueError("pixels must be %s = (iy, ix), got %s" % (want, np.shape(pixels)))
        pix_i = pix.astype(np.int64)
        if not np.array_equal(pix_i, pix) or pix_i.min() < 0 or pix_i.max() >= hm:
            raise ValueError("pixels must be integer (iy, ix) inside the %d x %d heightmap" % (hm, hm))
        return pix_i, listed

    @staticmethod
    def _read_q_values(eng, q, n_maps, aff, hm, K, pix, stream):
        """One smg_scene_values on the one-channel maps q [n_maps, 1, OH, OW] -> float32 [n_maps, K] on the device."""
        out = torch.empty((n_maps, K), dtype=torch.float32, device=q.device)
        eng.scene_values(q.data_ptr(), q.shape[2] * q.shape[3], n_maps, aff, hm, K, pix.data_ptr(), out.data_ptr(), stream)
        return out

    @staticmethod
    def _class_values_reader(what, cls, logits):
        """read(eng, q, n_maps, aff, hm, K, pix, stream) on the logit maps q [n_maps, 3, OH, OW] -> float32 [n_maps, 3, K], or
        [n_maps, K] for one `cls`: the probabilities by one smg_scene_class_values, or with `logits` the interpolated logits by one
        smg_scene_values per class plane (as forward_scene_class_maps uses smg_scene_maps)."""
        if cls is not None and cls not in (0, 1, 2):
            raise ValueError("%s: cls must be None (all three), 0, 1 or 2" % what)

        def read(eng, q, n_maps, aff, hm, K, pix, stream):
            OH, OW = q.shape[2], q.shape[3]
            if logits:
                planes = (0, 1, 2) if cls is None else (cls,)
                out = torch.empty((len(planes), n_maps, K), dtype=torch.float32, device=q.device)
                for k, c in enumerate(planes):
                    eng.scene_values(q[:, c].data_ptr(), 3 * OH * OW, n_maps, aff, hm, K, pix.data_ptr(), out[k].data_ptr(), stream)
                return out.permute(1, 0, 2).contiguous() if cls is None else out[0]
            out = torch.empty((n_maps, 3, K) if cls is None else (n_maps, K), dtype=torch.float32, device=q.device)
            eng.scene_class_values(q.data_ptr(), n_maps, aff, hm, -1 if cls is None else cls, K, pix.data_ptr(), out.data_ptr(), stream)
            return out
        return read

    @staticmethod
    def _values_out(out, return_device):
        return out if return_device else out.cpu().numpy().astype(np.float64)

    def _scene_values_sweep(self, model, depth_heightmap, pixels, style, specific_rotation, forward, read, return_device):
        """The body of scene_values and scene_class_values (the caller has checked method and geometry): the pixels checked and
        uploaded, `forward()` - which leaves its maps in self._last_q -, one `read` of all R maps at the same K points."""
        hm = int(np.shape(depth_heightmap)[-1])
        pix, _ = self._scene_value_pixels(pixels, None, hm)
        model._require_gpu()
        rots = self._scene_rotations(model, style, specific_rotation)
        pix_dev = _i32_on(model._flat_params.device, np.repeat(pix, len(rots), axis=0))
        forward()
        q = self._last_q
        eng, aff, _, stream = self._scene_call(model, q, depth_heightmap, rots)
        return self._values_out(read(eng, q, len(rots), aff, hm, pix.shape[1], pix_dev, stream), return_device)

    def _scene_values_objects(self, what, depth_heightmap, mask_depth, pixels, style, is_target, read, return_device):
        """The body of scene_object_values and scene_class_object_values: _object_maps' one engine call, one `read` over the n * R
        maps with object k's points repeated for its R maps -> [n, R, ..., K], the K axis dropped where the caller gave [n, 2]."""
        if style not in (0, 1):
            raise ValueError("%s: styles 0 (grasp) and 1 (suction)" % what)
        model = self.model_target if is_target else self.model
        n, hm = int(np.shape(mask_depth)[0]), int(np.shape(depth_heightmap)[-1])
        pix, listed = self._scene_value_pixels(pixels, n, hm)
        model._require_gpu()
        R = model.snum_rotations if style == 1 else model.gnum_rotations
        pix_dev = _i32_on(model._flat_params.device, np.repeat(pix, R, axis=0))
        model, q, _, n, R = self._object_maps(what, depth_heightmap, mask_depth, style, is_target)
        self._keep_object_q("grasp" if style == 0 else "suction", q)
        eng, aff, _, stream = self._scene_call(model, q, depth_heightmap, [(r, R) for k in range(n) for r in range(R)])
        out = read(eng, q, n * R, aff, hm, pix.shape[1], pix_dev, stream)
        out = out.reshape((n, R) + tuple(out.shape[1:]))
        return self._values_out(out if listed else out[..., 0], return_device)

    def _scene_values_pairs(self, depth_heightmap, mask_depth, pixels, is_target, read, return_device):
        """The body of scene_object_pair_values and scene_class_object_pair_values: _object_pair_maps' one engine call (style 2,
        rotation 0) and one `read` over the n_pairs maps -> ([n_pairs, ..., K] - the K axis dropped for [n_pairs, 2] -, [(g, s)]).
        With fewer than two objects nothing runs and the values are empty."""
        model = self.model_target if is_target else self.model
        n, hm = int(np.shape(mask_depth)[0]), int(np.shape(depth_heightmap)[-1])
        n_pairs = n * (n - 1) // 2
        if not n_pairs:
            dev = model._flat_params.device
            return torch.empty(0, dtype=torch.float32, device=dev) if return_device else np.empty(0, dtype=np.float64), []
        pix, listed = self._scene_value_pixels(pixels, n_pairs, hm)
        model._require_gpu()
        pix_dev = _i32_on(model._flat_params.device, pix)
        model, q, _, idx = self._object_pair_maps(depth_heightmap, mask_depth, is_target)
        self._keep_object_q("pairs", q)
        eng, aff, _, stream = self._scene_call(model, q, depth_heightmap, [(0, model.gnum_rotations)] * n_pairs)
        out = read(eng, q, n_pairs, aff, hm, pix.shape[1], pix_dev, stream)
        return self._values_out(out if listed else out[..., 0], return_device), idx

    def _keep_object_q(self, name, q):
        """self._last_object_q[name] = q, beside what best_scene_actions / best_scene_class_actions left there."""
        kept = dict(getattr(self, "_last_object_q", None) or {})
        kept[name] = q
        self._last_object_q = kept

    def scene_values(self, depth_heightmap, m_depth_heightmap, pixels, style=0, is_target=False, specific_rotation=-1, return_device=False):
        """forward_scene read at LISTED heightmap pixels: `pixels` [K, 2] = (iy, ix), or one (iy, ix) -> float64 [R, K] (or the
        float32 device tensor), equal to forward_scene(...)[:, iy, ix] bit for bit - forward_dense's engine call, rotation choice
        and BN bookkeeping, then one smg_scene_values: R * K floats are written instead of R * hm * hm.  A pixel without a window
        of the head in a rotation is -inf there and raises nothing.  The maps stay in self._last_q.  With is_target and a specific
        rotation this is the reference's target forward of code/trainer.py:255-270 plus one point.  Reinforcement method,
        heightmaps larger than 224^2."""
        self._require_scene("scene_values", depth_heightmap)
        return self._scene_values_sweep(
            self.model_target if is_target else self.model, depth_heightmap, pixels, style, specific_rotation,
            lambda: self.forward_dense(depth_heightmap, m_depth_heightmap, style, is_target, specific_rotation, return_device=True),
            self._read_q_values, return_device)

    def scene_object_values(self, depth_heightmap, mask_depth, pixels, style=0, is_target=False, return_device=False):
        """gra_conf / suc_conf of code/main.py:165-166 on a heightmap larger than 224^2, read at the caller's action points
        (masks_cter): `pixels` [n, 2] = object k's own (iy, ix), or [n, K, 2] -> float64 [n, R] or [n, R, K] (or the float32 device
        tensor).  forward_objects' one engine call (R + n trunk passes, the reference's BN sequence) and one smg_scene_values over
        the n * R maps, which stay in self._last_object_q["grasp" / "suction"].  -inf where a pixel has no window in a rotation.
        Styles 0 / 1, reinforcement method."""
        self._require_scene("scene_object_values", depth_heightmap)
        return self._scene_values_objects("scene_object_values", depth_heightmap, mask_depth, pixels, style, is_target,
                                          self._read_q_values, return_device)

    def scene_object_pair_values(self, depth_heightmap, mask_depth, pixels, is_target=False, return_device=False):
        """gs_conf of code/main.py:183-192 at given points: `pixels` [n_pairs, 2] or [n_pairs, K, 2] in forward_object_pairs' pair
        order -> (float64 [n_pairs] or [n_pairs, K] - or the float32 device tensor -, [(g, s)]); the maps stay in
        self._last_object_q["pairs"].  With fewer than two objects nothing runs.  Reinforcement method."""
        self._require_scene("scene_object_pair_values", depth_heightmap)
        return self._scene_values_pairs(depth_heightmap, mask_depth, pixels, is_target, self._read_q_values, return_device)

    def scene_class_values(self, depth_heightmap, m_depth_heightmap, pixels, style=0, specific_rotation=-1, cls=None, logits=False,
                           return_device=False):
        """forward_scene_class_maps read at LISTED heightmap pixels: `pixels` [K, 2] or one (iy, ix) -> float64 [R, 3, K] class
        probabilities, or [R, K] for one `cls` (or the float32 device tensor), bit for bit what forward_scene_class_maps gives at
        those pixels - one smg_scene_class_values, or with `logits` one smg_scene_values per class plane.  -inf where a pixel has
        no window in a rotation.  The logits stay in self._last_q.  Reactive method, heightmaps larger than 224^2."""
        self._require_scene_class("scene_class_values", depth_heightmap)
        return self._scene_values_sweep(
            self.model, depth_heightmap, pixels, style, specific_rotation,
            lambda: self.forward_class_maps(depth_heightmap, m_depth_heightmap, style, specific_rotation, logits=True, return_device=True),
            self._class_values_reader("scene_class_values", cls, logits), return_device)

    def scene_class_object_values(self, depth_heightmap, mask_depth, pixels, style=0, cls=0, logits=False, return_device=False):
        """scene_object_values for the reactive net: P(class `cls`) - or with `logits` the interpolated logit - of every (object,
        rotation) at object k's own points, `pixels` [n, 2] or [n, K, 2] -> [n, R] or [n, R, K] ([n, R, 3(, K)] for cls None).  The
        logits stay in self._last_object_q["grasp" / "suction"]."""
        self._require_class_objects("scene_class_object_values", depth_heightmap, mask_depth)
        self._scene_geometry(np.shape(depth_heightmap)[-1])
        return self._scene_values_objects("scene_class_object_values", depth_heightmap, mask_depth, pixels, style, False,
                                          self._class_values_reader("scene_class_object_values", cls, logits), return_device)

    def scene_class_object_pair_values(self, depth_heightmap, mask_depth, pixels, cls=0, logits=False, return_device=False):
        """scene_object_pair_values for the reactive net: (P(class `cls`) or the logit of every pair's style-2 map at its points,
        [(g, s)]).  The logits stay in self._last_object_q["pairs"]."""
        self._require_class_objects("scene_class_object_pair_values", depth_heightmap, mask_depth)
        self._scene_geometry(np.shape(depth_heightmap)[-1])
        return self._scene_values_pairs(depth_heightmap, mask_depth, pixels, False,
                                        self._class_values_reader("scene_class_object_pair_values", cls, logits), return_device)

    # ---- the collapsed map: per heightmap pixel the best value over the rotations and the rotation that gives it -----------------
    @staticmethod
    def _best_maps_out(val, arg, rotations, return_device):
        """The kernel's (value, map index) pair -> (conf, rotation): `rotations` = the rotation of every map of the call, looked
        up on the device (index -1, no candidate, stays -1).  Host: float64 and int32; device: the float32 and int32 tensors."""
        table = torch.tensor([-1] + [int(r) for r in rotations], dtype=torch.int32, device=arg.device)
        rot = table[(arg + 1).long()]
        if return_device:
            return val, rot
        return val.cpu().numpy().astype(np.float64), rot.cpu().numpy()

    def _best_rotation_sweep(self, what, model, depth_heightmap, style, forward, best_maps, return_device):
        """The body of best_rotation_map and best_rotation_class_map (the caller has checked method and geometry): `forward()` -
        the sweep's one engine call, maps [R, ...] on the device - and one best_maps(engine, q, R, affines, hm, masks None, mask_a,
        mask_b, groups, n_groups 1, val pointer, arg pointer, stream) with every term -1: one group, no masks tensor."""
        if style not in (0, 1):
            raise ValueError("%s: styles 0 (grasp) and 1 (suction); style 2 evaluates rotation 0 alone, there is nothing to collapse" % what)
        q = forward()
        R = int(q.shape[0])
        rots = self._scene_rotations(model, style, -1)
        eng, aff, hm, stream = self._scene_call(model, q, depth_heightmap, rots)
        val = torch.empty((1, hm, hm), dtype=torch.float32, device=q.device)
        arg = torch.empty((1, hm, hm), dtype=torch.int32, device=q.device)
        best_maps(eng, q, R, aff, hm, None, [-1] * R, [-1] * R, [0] * R, 1, val.data_ptr(), arg.data_ptr(), stream)
        return self._best_maps_out(val[0], arg[0], [r for r, _ in rots], return_device)

    def _best_rotation_objects(self, what, depth_heightmap, mask_depth, style, is_target, on_object, best_maps, return_device):
        """The body of best_rotation_object_maps and best_rotation_class_object_maps: _object_maps' one engine call, then one
        best_maps over its n * R maps, object-major, the group = the object, on the masks tensor that forward used (on_object) or
        on every pixel (no masks tensor).  The maps stay in self._last_object_q["grasp" / "suction"]."""
        model, q, m, n, R = self._object_maps(what, depth_heightmap, mask_depth, style, is_target)
        self._keep_object_q("grasp" if style == 0 else "suction", q)
        eng, aff, hm, stream = self._scene_call(model, q, depth_heightmap, [(r, R) for k in range(n) for r in range(R)])
        val = torch.empty((n, hm, hm), dtype=torch.float32, device=q.device)
        arg = torch.empty((n, hm, hm), dtype=torch.int32, device=q.device)
        mask_a = [k for k in range(n) for r in range(R)] if on_object else [-1] * (n * R)
        best_maps(eng, q, n * R, aff, hm, m if on_object else None, mask_a, [-1] * (n * R), [j // R for j in range(n * R)], n,
                  val.data_ptr(), arg.data_ptr(), stream)
        return self._best_maps_out(val, arg, [r for k in range(n) for r in range(R)], return_device)

    @staticmethod
    def _q_best_maps(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, val, arg, stream):
        eng.scene_best_maps(q.data_ptr(), q.shape[-2] * q.shape[-1], n_maps, aff, hm, None if m is None else m.data_ptr(),
                            0 if m is None else int(m.shape[0]), mask_a, mask_b, group_of, groups, val, arg, stream)

    @staticmethod
    def _class_best_maps(cls):
        def best_maps(eng, q, n_maps, aff, hm, m, mask_a, mask_b, group_of, groups, val, arg, stream):
            eng.scene_class_best_maps(q.data_ptr(), n_maps, aff, hm, cls, None if m is None else m.data_ptr(),
                                      0 if m is None else int(m.shape[0]), mask_a, mask_b, group_of, groups, val, arg, stream)
        return best_maps

    def best_rotation_map(self, depth_heightmap, m_depth_heightmap, style=0, is_target=False, return_device=False):
        """The affordance picture of the sweep: for every heightmap pixel the best Q value over the rotations and the rotation that
        gives it -> (conf float64 [hm, hm], rotation int32 [hm, hm]), equal to forward_scene(...) reduced by max / argmax over
        axis 0 (the lowest rotation on ties, the first NaN wins); (-inf, -1) where no rotation has a window of the head.  One
        forward_dense sweep and one smg_scene_best_maps with one group and no masks: the R scene-frame maps are never written.  A
        caller multiplies a per-pixel prior of its own - reachability, clearance - into conf on the device (`return_device`: the
        float32 and int32 tensors) and picks from the product.  Styles 0 / 1: style 2 and the object pairs evaluate rotation 0
        alone, so there is nothing to collapse (forward_scene gives that one map).  Reinforcement method, heightmaps larger than
        224^2."""
        self._require_scene("best_rotation_map", depth_heightmap)
        return self._best_rotation_sweep(
            "best_rotation_map", self.model_target if is_target else self.model, depth_heightmap, style,
            lambda: self.forward_dense(depth_heightmap, m_depth_heightmap, style, is_target, return_device=True),
            self._q_best_maps, return_device)

    def best_rotation_object_maps(self, depth_heightmap, mask_depth, style=0, is_target=False, on_object=True, return_device=False):
        """best_rotation_map per object -> (conf float64 [n, hm, hm], rotation int32 [n, hm, hm]): forward_objects_dense's single
        engine call and one smg_scene_best_maps over its n * R maps, the group = the object; the n * R scene-frame maps are never
        written.  on_object restricts object k to its own pixels (mask_depth[k] != 0), read from the masks tensor the forward used;
        False gives every pixel with a window.  Elsewhere the pair is (-inf, -1).  The maximum of conf[k] is best_scene_actions'
        per_object confidence of object k.  The maps stay in self._last_object_q["grasp" / "suction"], as after
        best_scene_actions.  Styles 0 / 1 (the pairs of style 2 have one rotation: nothing to collapse).  Reinforcement method,
        heightmaps larger than 224^2."""
        self._require_scene("best_rotation_object_maps", depth_heightmap)
        return self._best_rotation_objects("best_rotation_object_maps", depth_heightmap, mask_depth, style, is_target, on_object,
                                           self._q_best_maps, return_device)

    def best_rotation_class_map(self, depth_heightmap, m_depth_heightmap, style=0, cls=0, return_device=False):
        """best_rotation_map for the reactive net: per heightmap pixel the largest P(class `cls`) over the rotations - the logits
        interpolated, the softmax at the pixel, forward_scene_class_maps(cls=cls) reduced by max / argmax over axis 0 - and its
        rotation.  One forward_class_maps sweep, one smg_scene_class_best_maps.  There is no is_target: the reactive method has no
        target net.  Styles 0 / 1, cls in {0, 1, 2}, heightmaps larger than 224^2."""
        self._require_scene_class("best_rotation_class_map", depth_heightmap)
        if cls not in (0, 1, 2):
            raise ValueError("best_rotation_class_map: cls must be 0, 1 or 2")
        return self._best_rotation_sweep(
            "best_rotation_class_map", self.model, depth_heightmap, style,
            lambda: self.forward_class_maps(depth_heightmap, m_depth_heightmap, style, logits=True, return_device=True),
            self._class_best_maps(cls), return_device)

    def best_rotation_class_object_maps(self, depth_heightmap, mask_depth, style=0, on_object=True, cls=0, return_device=False):
        """best_rotation_object_maps for the reactive net: forward_class_objects' single engine call and one
        smg_scene_class_best_maps on its logits; conf is P(class `cls`).  The method and geometry refusals are
        best_scene_class_actions'; the logits stay in self._last_object_q["grasp" / "suction"]."""
        self._require_class_objects("best_rotation_class_object_maps", depth_heightmap, mask_depth)
        if cls not in (0, 1, 2):
            raise ValueError("best_rotation_class_object_maps: cls must be 0, 1 or 2")
        self._scene_geometry(np.shape(depth_heightmap)[-1])
        return self._best_rotation_objects("best_rotation_class_object_maps", depth_heightmap, mask_depth, style, False, on_object,
                                           self._class_best_maps(cls), return_device)

    # ---- the two calls that close the loop of code/main.py on a heightmap larger than 224^2 --------------------------------------
    @staticmethod
    def _scene_action(what, best, action, depth_heightmap, mask_depth):
        """The action `best` (best_scene_actions' or best_scene_class_actions' dict) names for the primitive `action` ->
        (masked heightmap, style, rotation, pixel): 'grasp' bestg_id = (k, r) and bestg_pixel on depth * mask[k]; 'suction' the
        bests_ keys; 'grasp_then_suction' bestgs_num = (g, s) and bestgs_pixel on depth * (mask[g] + mask[s]), rotation 0."""
        if action not in _ACTION_STYLE:
            raise ValueError("%s: unknown primitive %r" % (what, action))
        style = _ACTION_STYLE[action]
        key = ("bestg_id", "bests_id", "bestgs_num")[style]
        pixel = None if best is None else best.get(("bestg_pixel", "bests_pixel", "bestgs_pixel")[style])
        ids = None if best is None else best.get(key)
        if ids is None or pixel is None:
            raise ValueError("%s: best[%r] is None - best_scene_actions found no %s action in this scene" % (what, key, action))
        depth = np.asarray(depth_heightmap)
        if style == 2:
            return depth * (mask_depth[ids[0]] + mask_depth[ids[1]]), 2, 0, tuple(pixel)
        return depth * mask_depth[ids[0]], style, int(ids[1]), tuple(pixel)

    def get_label_value_scene(self, primitive_action, objects_number, suction_success, grasp_success, gs_success,
                              depth_heightmap, mask_depth, best, exploit_action):
        """get_label_value (code/trainer.py:212-274, code/main.py:317) on a heightmap larger than 224^2, with `best` the dict
        best_scene_actions returned for the current scene.  Reinforcement: rewards and the two zero-future cases are
        get_label_value's; otherwise the future reward is the TARGET net's value at the action the online net chose for
        `exploit_action` - object(s), rotation and pixel from `best` (_scene_action), one scene_values(..., is_target=True,
        specific_rotation=r) at that one pixel: the reference's two-stream, one-rotation target forward plus one point.  A None
        id for the chosen primitive raises ValueError.  Prints the reference's line, returns (expected_reward, current_reward).
        Reactive: get_label_value's (label_value, success_value); no forward runs and `best` may be None."""
        if self.method == 'reactive':
            return self._class_label(primitive_action, suction_success, grasp_success, gs_success)
        current_reward, no_future = self._reward_now(primitive_action, objects_number, suction_success, grasp_success, gs_success)
        if no_future:
            future_reward = 0
        else:
            m, style, rot, pixel = self._scene_action("get_label_value_scene", best, exploit_action, depth_heightmap, mask_depth)
            future_reward = self.scene_values(depth_heightmap, m, [pixel], style, is_target=True, specific_rotation=rot)[0, 0]
        expected_reward = current_reward + self.future_reward_discount * future_reward
        print('Expected reward: %f + %f x %f = %f' % (current_reward, self.future_reward_discount, future_reward, expected_reward))
        return expected_reward, current_reward

    def get_label_value_scene_soft(self, primitive_action, objects_number, suction_success, grasp_success, gs_success,
                                   depth_heightmap, mask_depth, temperature, kind, is_ets=True):
        """get_label_value_scene with a bootstrap that is consistent with Boltzmann exploration at `temperature` (reinforcement
        method only, else ValueError).  Rewards and the two zero-future cases are get_label_value_scene's; otherwise the future
        reward comes from the TARGET net's policy over ALL actions of the scene - scene_policy_stats(is_target=True, joint=True),
        its primitives merged (merge_policy_stats) -: kind "expected" = the Boltzmann-weighted expectation of Q, the merged mean
        (expected SARSA); kind "mellowmax" = temperature * (lse - log count), the non-expansive soft maximum, which lies between
        the arithmetic mean of the target's Q and that expectation.  Prints the reference's line, returns (expected_reward, current_reward)."""
        if self.method != 'reinforcement':
            raise ValueError("get_label_value_scene_soft: the soft bootstrap needs method == 'reinforcement'")
        if kind not in ("expected", "mellowmax"):
            raise ValueError("get_label_value_scene_soft: kind must be 'expected' or 'mellowmax'")
        if not np.isscalar(temperature):
            raise ValueError("get_label_value_scene_soft: one temperature")
        current_reward, no_future = self._reward_now(primitive_action, objects_number, suction_success, grasp_success, gs_success)
        if no_future:
            future_reward = 0
        else:
            stats = self.scene_policy_stats(depth_heightmap, mask_depth, temperature, is_ets=is_ets, is_target=True, joint=True)
            merged = self.merge_policy_stats(*(stats[name] for name in ("grasp", "suction", "pairs")))
            future_reward = float(merged["mean" if kind == "expected" else "mellowmax"][0])
        expected_reward = current_reward + self.future_reward_discount * future_reward
        print('Expected reward: %f + %f x %f = %f' % (current_reward, self.future_reward_discount, future_reward, expected_reward))
        return expected_reward, current_reward

    def backprop_scene(self, depth_heightmap, primitive_action, best, label_value, objects_mask):
        """backprop (code/trainer.py:334-384, code/main.py:338) on a heightmap larger than 224^2: the reference's one-sample step
        on the EXECUTED action - object(s), rotation and heightmap pixel taken from `best` (_scene_action) - as one
        train_batch_scene_pixels (reinforcement, Huber against `label_value`) or train_batch_scene_class_pixels (reactive, the
        class label) with one sample and one pixel.  `objects_mask` is [n, H, H] or [n, H, H, 1] and is not reshaped in place.
        Prints the reference's line and returns the loss as a 0-d array."""
        mask_depth = np.asarray(objects_mask)
        if mask_depth.ndim == 4:
            mask_depth = mask_depth[..., 0]
        m, style, rot, pixel = self._scene_action("backprop_scene", best, primitive_action, depth_heightmap, mask_depth)
        step = self.train_batch_scene_pixels if self.method == 'reinforcement' else self.train_batch_scene_class_pixels
        loss = step(depth_heightmap, m, style, [rot], [[pixel]], [label_value])
        loss_value = np.asarray(loss.cpu().numpy()[0])
        print('Training loss: %f' % (loss_value))
        return loss_value

    def backprop_scene_policy(self, depth_heightmap, primitive_action, best, objects_mask, temperature, weight=1.0, entropy_weight=0.0):
        """The policy step on the EXECUTED action: `best` is the dict best_scene_actions, ranked_to_best or the sampled forms
        return, decoded by _scene_action.  The executed object's masked heightmap goes through all R rotations (rotation 0 alone
        for 'grasp_then_suction'); they form ONE group, selected by the object's mask (the union of both for a pair), whose action
        is the executed (rotation, pixel): one train_batch_scene_policy.  `weight` is the NLL weight - 1 clones a demonstration,
        an advantage makes it the policy-gradient step -, `entropy_weight` the entropy bonus, `temperature` the policy's.
        `objects_mask` is [n, H, H] or [n, H, H, 1] and is not reshaped in place.  Reinforcement method only.  Prints the
        reference's line and returns the loss as a 0-d array."""
        if self.method != 'reinforcement':
            raise ValueError("backprop_scene_policy: reinforcement method only (the reactive net is trained by its class labels)")
        mask_depth = np.asarray(objects_mask)
        if mask_depth.ndim == 4:
            mask_depth = mask_depth[..., 0]
        m, style, rot, pixel = self._scene_action("backprop_scene_policy", best, primitive_action, depth_heightmap, mask_depth)
        ids = best[("bestg_id", "bests_id", "bestgs_num")[style]]
        if style == 2:
            masks, rotations, which = np.stack([mask_depth[ids[0]], mask_depth[ids[1]]]), [0], (0, 1)
        else:
            masks, rotations, which = mask_depth[ids[0]][None], list(range(self.model.gnum_rotations)), 0
            if not 0 <= rot < len(rotations):
                raise ValueError("backprop_scene_policy: rotation %d is outside the %d trained rotations" % (rot, len(rotations)))
        loss = self.train_batch_scene_policy(depth_heightmap, m, style, rotations, masks, [which] * len(rotations), [0] * len(rotations),
                                             [(0 if style == 2 else rot, pixel)], temperature, [weight], [entropy_weight])
        loss_value = np.asarray(loss.cpu().numpy()[0])
        print('Training loss: %f' % (loss_value))
        return loss_value

    # The single-sample step of Trainer.backprop as ONE replayed hipGraph (smg_train_step_graph): ~560 launches of 2-20 us each are
    # enqueued by one hipGraphLaunch instead of one by one (same results, bit for bit at zero learning rate).  It saves a little host time
    # (1.8 ms per step instead of 2.3) and costs latency: the graph's ~560 dependent nodes execute no faster than the same launches from
    # two streams whose host stays ahead of the GPU - 6.6-6.8 ms per step as a graph against 5.5 ms as separate calls (bench.py;
    # splitting the graph so that its launch cost hides changed nothing).  The reference's loop reads the loss of every step before it
    # continues (latency, not throughput), so the separate calls are the default.
    use_step_graph = False

    def _train_step_graph(self, depth_heightmap, m_depth_heightmap, style, rotation, label_value):
        t_host = time.perf_counter()
        model = self.model
        model._require_gpu()
        dev = model._flat_params.device
        hm = np.stack([np.asarray(depth_heightmap, dtype=np.float64), np.asarray(m_depth_heightmap, dtype=np.float64)])
        if hm.ndim != 3 or hm.shape[1] != hm.shape[2]:
            raise ValueError("heightmaps must be square 2-D arrays")
        st = getattr(self, "_step_state", None)
        if st is None or st["model"] is not model or st["hm"].shape != hm.shape or st["hm"].device != dev:
            # persistent device buffers: the captured graph is keyed on their addresses
            st = self._step_state = dict(model=model, hm=torch.empty(hm.shape, dtype=torch.float64, device=dev),
                                         label=torch.empty(1, dtype=torch.float32, device=dev), loss=torch.empty(1, dtype=torch.float32, device=dev),
                                         q=None, dq=None)
        if st["q"] is None or st["q"].shape[1] != model.HEAD_OUT:
            st["q"] = torch.empty((1, model.HEAD_OUT, 1, 1), dtype=torch.float32, device=dev)
            st["dq"] = torch.empty_like(st["q"])
        st["hm"].copy_(torch.from_numpy(np.ascontiguousarray(hm)))
        st["label"].fill_(float(label_value))
        key = (STYLE_TRUNK[style], STYLE_HEAD[style])
        if model._graph_exposed != key:
            self.optimizer.zero_grad()          # the reference's zero_grad: every p.grad dropped (the graph zeroes its own two ranges)
        rot = 0 if style == 2 else rotation
        model.train_step_graph(style, rot, model.gnum_rotations, st["hm"], st["label"], st["loss"], st["q"], st["dq"], self.optimizer,
                               0 if self.method == 'reinforcement' else 1, mean=self.image_mean, std=self.image_std)
        if model._graph_exposed != key:
            model.expose_grads(*key)
            model._graph_exposed = key
        setattr(model, ("gra_prob", "suc_prob", "gs_prob")[style], st["q"])
        self.last_enqueue_ms = (time.perf_counter() - t_host) * 1e3        # host time of the step up to the loss read-back (bench.py)
        return np.asarray(st["loss"].cpu().numpy()[0])

    def train_step(self, depth_heightmap, m_depth_heightmap, style, rotation, label_value):
        """zero_grad -> forward (branch C) -> loss -> backward -> Adam, all on the device;
        the only host synchronisation is reading the loss back (as code/trainer.py:352 does)."""
        if self.use_step_graph and np.shape(depth_heightmap)[-1] == 224:      # (S = 640: one Q value per sample; larger inputs keep the eager calls)
            return self._train_step_graph(depth_heightmap, m_depth_heightmap, style, rotation, label_value)
        t_host = time.perf_counter()
        model = self.model
        self.optimizer.zero_grad()
        # (the label goes up BEFORE the forward is enqueued: a pageable host-to-device copy returns only when the stream has reached it -
        #  behind the forward it held the host for the forward's ~1.5 ms, with the backward not yet enqueued)
        labels = torch.tensor([float(label_value)], dtype=torch.float32, device=model._flat_params.device)
        q = self._evaluate(model, depth_heightmap, m_depth_heightmap, style, False, rotation)
        dev = q.device
        eng, token, trunk_id, head_id = model._saved
        stream = torch.cuda.current_stream(dev).cuda_stream
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dq = torch.empty_like(q)
        eng.loss(0 if self.method == 'reinforcement' else 1, q.data_ptr(), labels.data_ptr(), 1, loss.data_ptr(), dq.data_ptr(), stream)
        model._engine_backward(token, dq)
        self.optimizer.step()
        setattr(model, ("gra_prob", "suc_prob", "gs_prob")[style], q)
        self.last_enqueue_ms = (time.perf_counter() - t_host) * 1e3
        return np.asarray(loss.cpu().numpy()[0])
