"""GraphPointwiseDataset / GraphRankingDataset (reference datasets/gnn_datasets.py): samples are node ids of the graph."""
import numpy as np
import torch

from .base import PointwiseDataset, RankingDataset, ResidentInputs


class GraphPointwiseDataset(PointwiseDataset):
    def __init__(self, file_or_frame, graph_content_provider):
        super().__init__(file_or_frame)
        self.gcp = graph_content_provider
        # node ids for the whole file at once (the reference resolves them per sample through two dicts)
        self._unode = np.asarray(self.gcp.get_user_nodeID(self._u))
        self._inode = np.asarray(self.gcp.get_item_nodeID(self._i))

    def __getitem__(self, item):
        return self._unode[item], self._inode[item], self._r[item]

    def resident_inputs(self, device=None, batch_size=None):
        return ResidentInputs((torch.as_tensor(self._unode, dtype=torch.int64), torch.as_tensor(self._inode, dtype=torch.int64)), self._targets())

    def get_graph(self, device):
        return self.gcp.get_graph().to(device)

    def use_collate(self):
        def collate(batch):
            u, i, t = zip(*batch)
            return torch.as_tensor(np.asarray(u), dtype=torch.int64), torch.as_tensor(np.asarray(i), dtype=torch.int64), torch.as_tensor(np.asarray(t), dtype=torch.float32)
        return collate

    @staticmethod
    def do_forward(model, batch, device, graph, *args):
        userIds, itemIds, y_batch = batch
        return model(graph.to(device), userIds.long().to(device), itemIds.long().to(device), device, *args), y_batch


class GraphRankingDataset(RankingDataset):
    """Reference gnn_datasets.py:32-57: samples are (user node, positive node, negative node) with the negative drawn as the
    reference draws it; node ids for the whole file (negatives included) are resolved once, at construction."""

    def __init__(self, file_or_frame, graph_content_provider):
        super().__init__(file_or_frame)
        self.gcp = graph_content_provider
        self._unode = np.asarray(self.gcp.get_user_nodeID(self._u))
        self._pnode = np.asarray(self.gcp.get_item_nodeID(self._pos))
        self._nnode = np.asarray(self.gcp.get_item_nodeID(self._neg_ids))

    def __getitem__(self, item):
        # base.py:72-78's draw (np.random.choice over the row's entries: the same RNG calls whether it picks ids or positions)
        s, e = self._rowptr[item], self._rowptr[item + 1]
        k = s + np.random.choice(e - s, p=self._negative_sampling_probs(np.array(self._neg_r[s:e])))
        return self._unode[item], self._pnode[item], self._nnode[k]

    def resident_pairs(self, device=None):
        if device is None or torch.device(device).type != "cuda":
            return None
        if str(device) in self._resident:
            return self._resident[str(device)]
        dev = torch.device(device)
        return self._resident_pairs(dev, torch.as_tensor(self._unode, dtype=torch.int64).to(dev),
                                    torch.as_tensor(self._pnode, dtype=torch.int64).to(dev), torch.as_tensor(self._nnode, dtype=torch.int32).to(dev))

    def get_graph(self, device):
        return self.gcp.get_graph().to(device)

    def use_collate(self):
        def collate(batch):
            return tuple(torch.as_tensor(np.asarray(col), dtype=torch.int64) for col in zip(*batch))
        return collate

    @staticmethod
    def do_forward(model, batch, device, graph, *args):
        """Two model calls, as the reference makes them: in training each masks its own target edges (mask_targets)."""
        userIds, item1Ids, item2Ids = batch
        out1 = model(graph.to(device), userIds.long().to(device), item1Ids.long().to(device), device, *args)
        out2 = model(graph.to(device), userIds.long().to(device), item2Ids.long().to(device), device, *args)
        return out1, out2
