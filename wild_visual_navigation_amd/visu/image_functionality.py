"""The storing half of the reference's plot decorator (visu/image_functionality.py): ``store=`` / ``tag=`` / ``epoch=`` /
``store_folder=`` keyword arguments of every plot method, file ``{epoch}_{tag}.png`` under the visualizer's ``p_visu``.

Two differences from the reference: the PNG is written with PIL (imageio is not a dependency), and the plot is evaluated ONCE
(the reference's wrapper calls the plot function a second time for its return value).  The ``log`` path (neptune / wandb /
tensorboard through cv2) is outside this package: ``not_log`` is accepted and ignored."""
import functools
import os


def image_functionality(func):
    @functools.wraps(func)
    def wrap(self, *args, **kwargs):
        img = func(self, *args, **kwargs)
        store = kwargs["store"] if kwargs.get("store", None) is not None else self._store
        if store:
            from .._lib import WvnError

            if self._p_visu is None:
                raise WvnError("store=True needs a visualizer constructed with p_visu (the folder the pictures go to)")
            tag = kwargs.get("tag", "")
            epoch = kwargs["epoch"] if kwargs.get("epoch", None) is not None else self._epoch
            folder = self._p_visu
            if kwargs.get("store_folder", None) is not None:
                folder = str(os.path.join(self._p_visu, kwargs["store_folder"]))
                os.makedirs(folder, exist_ok=True)
            try:
                from PIL import Image
            except ImportError as e:
                raise WvnError("store=True writes the PNG with PIL (Pillow), which is not installed") from e
            arr = img.cpu().numpy() if hasattr(img, "cpu") else img
            Image.fromarray(arr).save(os.path.join(folder, f"{epoch}_{tag}.png"))
        return img

    return wrap
