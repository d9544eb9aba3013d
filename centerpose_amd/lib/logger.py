"""``Logger(opt)`` of the reference's entry points (lib/logger.py): the options as ``opt.txt`` and a running ``log.txt``,
both under ``opt.save_dir``; scalars go to TensorBoard when it can be imported (``<save_dir>/logs``), otherwise
``scalar_summary`` does nothing.  ``img_summary`` always does nothing: the trainer produces no debug pictures."""
import os
import sys
import time

import torch

try:
    import torch.utils.tensorboard as _tensorboard
except Exception:  # tensorboard is an optional package
    _tensorboard = None

USE_TENSORBOARD = _tensorboard is not None


class Logger(object):
    def __init__(self, opt):
        os.makedirs(opt.save_dir, exist_ok=True)
        if getattr(opt, 'debug_dir', None):
            os.makedirs(opt.debug_dir, exist_ok=True)
        fields = {name: getattr(opt, name) for name in dir(opt) if not name.startswith('_')}
        with open(os.path.join(opt.save_dir, 'opt.txt'), 'wt') as f:
            f.write('==> torch version: {}\n'.format(torch.__version__))
            f.write('==> Cmd:\n{}\n==> Opt:\n'.format(sys.argv))
            for k, v in sorted(fields.items()):
                f.write('  %s: %s\n' % (k, v))
        self.writer = _tensorboard.SummaryWriter(log_dir=os.path.join(opt.save_dir, 'logs')) if USE_TENSORBOARD else None
        self.log = open(os.path.join(opt.save_dir, 'log.txt'), 'w')
        self.start_line = True

    def write(self, txt):
        """Appends ``txt``; a new line starts with the time, and a text with a line break flushes the file."""
        self.log.write('{}: {}'.format(time.strftime('%Y-%m-%d-%H-%M'), txt) if self.start_line else txt)
        self.start_line = '\n' in txt
        if self.start_line:
            self.log.flush()

    def close(self):
        self.log.close()
        if self.writer is not None:
            self.writer.close()

    def scalar_summary(self, tag, value, step):
        if self.writer is not None:
            self.writer.add_scalar(tag, value, step)

    def img_summary(self, tag, value_list, step):
        pass
