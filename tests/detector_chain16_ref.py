"""tests/detector_chain_ref.py's Chain with section 32's storage points in the three heads as well: the reference of a
training step whose trunk AND heads keep bfloat16 rows under float32 master weights.  detector_chain_ref.py is imported, not edited: the trunk, the
FPN, both RoIAligns, the targets and the five losses are its own; only the five head callables are restated here, layer by layer over the same
torch.nn modules (so the parameters, their names and their gradients are the base class's), with a straight-through rounding (_Stored) at
  * the packed input rows of a head (the value; the gradient that leaves a head's first layer is float32 and is not rounded),
  * every head weight as packed (its .grad stays float32: the master weights),
  * every stored row: the output of every layer but a head's last (the value, and the gradient that arrives there: a data-gradient launch
    rounds once after the mask, and the mask of a ReLU commutes with the rounding),
  * the gradient arriving at each raw output (the gradient pack).
heads_storage=None gives the base class's heads back, value for value."""
import torch
import torch.nn.functional as F

import detector_chain_ref as cr


class Chain16(cr.Chain):
    def __init__(self, sd, train_from_stage=2, dtype=torch.float64, storage='bfloat16', heads_storage='bfloat16', mutate=None):
        super().__init__(sd, train_from_stage, dtype, storage, mutate)
        if heads_storage not in (None, 'bfloat16'):
            raise ValueError(f'heads_storage is None or bfloat16, got {heads_storage!r}')
        self.heads_storage = heads_storage
        if heads_storage:
            self.modules = dict(self.heads)
            self.heads = dict(zip(cr.HEAD_PREFIXES, (self._rpn, self._box_head, self._box_predictor, self._mask_head, self._mask_predictor)))

    def _hs(self, x, fwd=True, bwd=True):
        return cr._Stored.apply(x, fwd, bwd)

    def _w(self, m):
        return self._hs(m.weight, True, False)

    def _hidden(self, name, v):
        """a stored row behind a ReLU; name: the module that reads it (detector_chain_ref.AFTER_RELU's kink)"""
        h = self._hs(torch.relu(v))
        self.kinks.append((name, h > 0))
        return h

    def _rpn(self, maps):
        m = self.modules['rpn.head']
        hidden = [self._hidden('rpn.head.cls_logits', F.conv2d(self._hs(f, True, False), self._w(m.conv), m.conv.bias, padding=1)) for f in maps]
        return ([self._hs(F.conv2d(h, self._w(m.cls_logits), m.cls_logits.bias), False, True) for h in hidden],
                [self._hs(F.conv2d(h, self._w(m.bbox_pred), m.bbox_pred.bias), False, True) for h in hidden])

    def _box_head(self, feats):
        m = self.modules['roi_heads.box_head']
        h6 = self._hidden('roi_heads.box_head.fc7', F.linear(self._hs(feats.flatten(1), True, False), self._w(m.fc6), m.fc6.bias))
        return self._hidden('roi_heads.box_predictor.cls_score', F.linear(h6, self._w(m.fc7), m.fc7.bias))

    def _box_predictor(self, h7):
        m = self.modules['roi_heads.box_predictor']
        return (self._hs(F.linear(h7, self._w(m.cls_score), m.cls_score.bias), False, True), self._hs(F.linear(h7, self._w(m.bbox_pred), m.bbox_pred.bias), False, True))

    def _mask_head(self, feats):
        m = self.modules['roi_heads.mask_head']
        x = self._hs(feats, True, False)
        readers = ('roi_heads.mask_head.mask_fcn2', 'roi_heads.mask_head.mask_fcn3', 'roi_heads.mask_head.mask_fcn4', 'roi_heads.mask_predictor.conv5_mask')
        for i, reader in enumerate(readers):
            conv = getattr(m, f'mask_fcn{i + 1}')
            x = self._hidden(reader, F.conv2d(x, self._w(conv), conv.bias, padding=1))
        return x

    def _mask_predictor(self, x):
        m = self.modules['roi_heads.mask_predictor']
        up = self._hidden('roi_heads.mask_predictor.mask_fcn_logits', F.conv_transpose2d(x, self._w(m.conv5_mask), m.conv5_mask.bias, stride=2))
        return self._hs(F.conv2d(up, self._w(m.mask_fcn_logits), m.mask_fcn_logits.bias), False, True)
