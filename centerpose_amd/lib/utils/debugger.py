"""``Debugger`` (utils/debugger.py): the result pictures of the demo, drawn by this library's own rasteriser.

The constructor arguments and the methods the detectors call are the reference's.  Each ``add_*`` appends to a per-image
log of drawing operations at the level of the reference's cv2 calls (``ops``: rectangle / circle / line / putText with the
integer coordinates np.int32 / int() give), and nothing is rasterised before an image is saved: ``render`` turns the log into
primitives (centerpose_amd/hip/draw.py) and draws them with ``hip.draw.draw_primitives`` on a CUDA device, or with the same
rule in numpy otherwise.  What differs from cv2's output is the rasteriser -- the coverage rule of csrc/draw_common.h, no
anti-aliasing, the library's 5 x 7 font at scale 2 for cv2's Hershey font at 0.5 -- not which things are drawn or in which order
(tests/test_draw_cpu.py pins that to the reference's call sequence).

Out of scope (each raises NotImplementedError naming this): the heat-map views of ``debug()`` -- gen_colormap,
gen_colormap_hp, add_blend_img, add_arrow, add_coco_hp_paper."""
import os

import numpy as np

from centerpose_amd.hip import _structs as S

TEXT_SCALE = S.DRAW_LABEL_SCALE  # integer glyph scale used where the reference asks cv2 for font scale 0.5


def _pack(bgr):
    return int(bgr[0]) | int(bgr[1]) << 8 | int(bgr[2]) << 16


def _trunc(v):
    """A coordinate as np.int32(...) / int() take it, towards zero; None when it is not finite or does not fit int32."""
    v = float(v)
    return int(v) if abs(v) < 2147483648.0 else None


def _in_range(*vs):
    return all(v is not None and S.DRAW_COORD_MIN <= v <= S.DRAW_COORD_MAX for v in vs)


class Debugger(object):
    def __init__(self, ipynb=False, theme='black', num_classes=-1, dataset=None, down_ratio=4, device=None):
        self.ipynb = ipynb
        self.imgs = {}
        self.ops = {}      # img_id -> [(name, ...)] in drawing order
        self.theme = theme
        self.device = device  # None: a CUDA device when there is one
        self.dim_scale = 1
        self.names = ['op']
        self.num_class = 1
        self.num_joints = 8
        self.edges = [[2, 4], [2, 6], [6, 8], [4, 8], [1, 2], [3, 4], [5, 6], [7, 8], [1, 3], [1, 5], [3, 7], [5, 7]]
        self.top_cross = [[3, 8], [4, 7]]
        self.front_cross = [[2, 8], [4, 6]]
        self.colors_hp = [(0, 0, 255), (0, 165, 255), (0, 255, 255), (0, 128, 0), (255, 0, 0), (130, 0, 75), (238, 130, 238),
                          (0, 0, 0), (255, 0, 0), (255, 0, 0), (255, 0, 0)]   # BGR
        self.down_ratio = down_ratio
        self.world_size = 64
        self.out_size = 384

    # ---- the log ----
    def add_img(self, img, img_id='default', revert_color=False):
        img = np.asarray(img)
        self.imgs[img_id] = (255 - img if revert_color else img).copy()
        self.ops[img_id] = []

    def _cat_colour(self, cat):
        if int(cat) != 0:
            raise NotImplementedError("Debugger: only category 0 has a colour here (the reference's colour table is not carried)")
        c = S.DRAW_CAT0['white' if self.theme == 'white' else 'black']
        return (c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF)

    def _text_size(self, txt):
        from centerpose_amd.hip import draw as hd

        return hd.text_size(txt, TEXT_SCALE)

    def add_coco_bbox(self, bbox, cat, conf=1, id=None, show_txt=True, img_id='default'):
        b = [_trunc(v) for v in bbox[:4]]
        c = self._cat_colour(cat)
        if not _in_range(*b):   # a non-finite or far-away corner withdraws the box and its label
            return
        height, width = self.imgs[img_id].shape[0], self.imgs[img_id].shape[1]
        b = [min(max(b[0], 0), width), min(max(b[1], 0), height), min(max(b[2], 0), width), min(max(b[3], 0), height)]
        if id is None:
            txt = '{}{:.1f}'.format(self.names[int(cat)], conf)
        else:
            txt = '{}{:.1f} ID:{}'.format(self.names[int(cat)], conf, id)
        cat_size = self._text_size(txt)
        ops = self.ops[img_id]
        ops.append(('rectangle', (b[0], b[1]), (b[2], b[3]), c, 2))
        if show_txt:
            ops.append(('rectangle', (b[0], b[1] - cat_size[1] - 2), (b[0] + cat_size[0], b[1] - 2), c, -1))
            ops.append(('putText', txt, (b[0], b[1] - 2), (0, 0, 0)))

    def add_obj_scale(self, bbox, scale, img_id='default', pred_flag='pred'):
        b = [_trunc(v) for v in bbox[:4]]
        if not _in_range(*b[:2]):
            return
        tag, top, bottom, base = {'pred': ('Pred', lambda h: h + 2, lambda h: 2 * h + 4, lambda h: 2 * h),
                                  'gt': ('GT', lambda h: 2, lambda h: h + 2, lambda h: h),
                                  'pnp': ('PnP', lambda h: 2, lambda h: h + 6, lambda h: h)}[pred_flag]
        txt = '{}:{:.3f}/{:.3f}/{:.3f}'.format(tag, scale[0], scale[1], scale[2])
        w, h = self._text_size(txt)
        ops = self.ops[img_id]
        ops.append(('rectangle', (b[0], b[1] + top(h)), (b[0] + w, b[1] + bottom(h)), (0, 0, 0), -1))
        ops.append(('putText', txt, (b[0], b[1] + base(h)), (255, 255, 255)))

    def add_coco_hp(self, points, img_id='default', pred_flag='pred', PAPER_DISPLAY=False):
        pts = [(_trunc(x), _trunc(y)) for x, y in np.asarray(points, np.float64).reshape(self.num_joints, 2)]
        ops = self.ops[img_id]
        for j in range(self.num_joints):
            if None in pts[j]:
                continue
            if not PAPER_DISPLAY:
                ops.append(('circle', pts[j], 5, self.colors_hp[j], -1))
            else:
                ops.append(('circle', pts[j], 10, (255, 255, 0), -1))

        def line(e, colour):
            a, c = pts[e[0] - 1], pts[e[1] - 1]
            if None in a or None in c or min(a) <= -10000 or min(c) <= -10000:
                return
            ops.append(('line', a, c, colour, 2))

        edge_color = {'pred': (0, 0, 255), 'gt': (0, 255, 0), 'pnp': (0, 0, 255), 'extra': (0, 165, 255)}[pred_flag]
        for e in self.edges:
            line(e, edge_color)
        edge_color = {'pred': (0, 0, 255), 'gt': (255, 255, 255), 'pnp': (0, 0, 0)}.get(pred_flag, edge_color)
        if not PAPER_DISPLAY:
            for e in self.front_cross:   # (the reference draws the top cross inside this loop: twice)
                line(e, edge_color)
                for t in self.top_cross:
                    line(t, edge_color)

    def add_axes(self, box, cam_intrinsic, img_id='default'):
        box = np.asarray(box, np.float64).reshape(9, 3)
        K = np.asarray(cam_intrinsic, np.float64).reshape(3, 3)
        N = 0.5
        pts = []
        for axes_point in [0, box[3] - box[1], box[2] - box[1], box[5] - box[1]]:
            vector = axes_point
            with np.errstate(all='ignore'):
                vector = vector / np.linalg.norm(vector) * N if np.linalg.norm(vector) != 0 else 0
                k_3d = (vector + box[0]).flatten()
                pp = np.matmul(K, k_3d.reshape(3, 1))
                pts.append((_trunc(pp[0, 0] / pp[2, 0]), _trunc(pp[1, 0] / pp[2, 0])))
        ops = self.ops[img_id]
        for end, colour in ((1, (0, 255, 0)), (2, (255, 0, 0)), (3, (0, 0, 255))):   # y green, z blue, x red
            if None not in pts[0] and None not in pts[end]:
                ops.append(('line', pts[0], pts[end], colour, 5))

    # ---- from the log to primitives and pixels ----
    def primitives(self, img_id='default'):
        """The image's log as primitive 8-tuples in drawing order (hip.draw.pack_primitives packs them)."""
        from centerpose_amd.hip import draw as hd

        out = []
        for op in self.ops[img_id]:
            if op[0] == 'rectangle':
                (x0, y0), (x1, y1), c, t = op[1:]
                out.append((S.DRAW_FILL if t < 0 else S.DRAW_RECT, x0, y0, x1, y1, max(t, 0), _pack(c), 0))
            elif op[0] == 'circle':
                (x, y), r, c, _ = op[1:]
                out.append((S.DRAW_DISC, x, y, 0, 0, r, _pack(c), 0))
            elif op[0] == 'line':
                (x0, y0), (x1, y1), c, t = op[1:]
                out.append((S.DRAW_SEGMENT, x0, y0, x1, y1, t, _pack(c), 0))
            else:  # putText: the origin is the text's bottom-left corner, a glyph's its cell's top-left
                txt, (x, y), c = op[1:]
                out += hd.text_primitives(txt, x, y - 7 * TEXT_SCALE, TEXT_SCALE, _pack(c))
        return out

    def render(self, img_id='default'):
        """The image with its log drawn: a new uint8 array [H, W, 3]."""
        import torch

        from centerpose_amd.hip import draw as hd

        img = np.ascontiguousarray(self.imgs[img_id], np.uint8)
        prims = self.primitives(img_id)
        if not prims or img.ndim != 3 or img.shape[2] != 3:
            return img.copy()
        dev = self.device if self.device is not None else (torch.device('cuda') if torch.cuda.is_available() else None)
        if dev is not None and torch.device(dev).type == 'cuda':
            frames = torch.from_numpy(img).to(dev)
            packed = torch.from_numpy(hd.pack_primitives(prims, len(prims))).to(dev)
            return hd.draw_primitives(frames, packed).cpu().numpy()
        return hd.rasterize_host(img.copy(), prims)

    def _stamp(self, txt, cat_h):
        for img_id, v in self.imgs.items():
            self.ops[img_id].append(('putText', txt, (5, v.shape[0] - cat_h), (255, 255, 255)))

    def _write(self, path, img_id):
        img = self.render(img_id)
        try:
            from cv2 import imwrite
        except ImportError:   # no cv2 (or a stand-in without imwrite): PIL writes the same pixels
            from PIL import Image
            Image.fromarray(img[:, :, ::-1] if img.ndim == 3 else img).save(path)
        else:
            imwrite(path, img)

    def show_all_imgs(self, pause=False, time=0):
        """No GUI here: the pictures are written by the save_* methods."""

    def save_all_imgs(self, path='./cache/debug/', prefix=''):
        for i in self.imgs:
            self._write(path + '/{}{}.png'.format(prefix, i), i)

    def save_all_imgs_eval(self, src_path, path='./cache/debug/', video_layout=False):
        file_id_name = src_path[src_path.rfind('_') + 1:]
        folder_name = src_path[:src_path.rfind('_')]
        txt = 'Frame:{}'.format(int(file_id_name))
        self._stamp(txt, self._text_size(txt)[1])
        for i in self.imgs:
            if video_layout:
                self._write(path + '/{}_{}.png'.format(file_id_name, i), i)
            else:
                self._write(path + '/{}_{}_{}.png'.format(folder_name, file_id_name, i), i)

    def save_all_imgs_demo(self, src_path, path='./cache/debug/'):
        file_id_name = os.path.splitext(os.path.basename(src_path))[0]
        if os.path.isdir(src_path):
            folder_name = src_path.split('/')[-2]
            if file_id_name.isnumeric():
                txt = 'Frame: {}'.format(int(file_id_name))
                self._stamp(txt, self._text_size(txt)[1])
            for i in self.imgs:
                self._write(path + '/{}_{}_{}.png'.format(folder_name, file_id_name, i), i)
        else:
            for i in self.imgs:
                self._write(path + '/{}_{}.png'.format(file_id_name, i), i)

    # ---- the heat-map views of debug(): out of scope ----
    def _out_of_scope(self, name):
        raise NotImplementedError("Debugger.%s: the heat-map debug views (debug 2 / 3) are out of scope of this library's "
                                  "drawing; only the result pictures are drawn" % name)

    def gen_colormap(self, *a, **k):
        self._out_of_scope('gen_colormap')

    def gen_colormap_hp(self, *a, **k):
        self._out_of_scope('gen_colormap_hp')

    def add_blend_img(self, *a, **k):
        self._out_of_scope('add_blend_img')

    def add_arrow(self, *a, **k):
        self._out_of_scope('add_arrow')

    def add_coco_hp_paper(self, *a, **k):
        self._out_of_scope('add_coco_hp_paper')
