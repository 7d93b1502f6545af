"""The real-world caller of ``Imagen.sample``: read a MinImagen *training directory*
(``parameters/*.json`` + ``state_dicts/`` or ``tmp/`` checkpoints), build the model, sample captions and write image files.
Mirrors the observable behaviour of minimagen/generate.py:12-173 (directory layout, file names, errors); sampling itself
runs on the HIP path of :class:`minimagen_amd.Imagen`."""
import json
import os
from datetime import datetime
from typing import List, Optional, Tuple

import torch

from .Imagen import Imagen
from .Unet import Unet


def _unet_index(name: str) -> int:
    return int(name.split("_")[1])


def load_params(directory: str) -> Tuple[List[dict], dict]:
    """generate.py:49-67: ``(unets_params, imagen_params)`` from ``<directory>/parameters``; the i-th list entry is the
    keyword dict of U-Net i (files ``unet_<i>_params_*.json``), the Imagen dict comes from ``imagen_params_*.json``."""
    pdir = os.path.join(directory, "parameters")
    names = os.listdir(pdir)

    def read(name):
        with open(os.path.join(pdir, name), "r") as fh:
            return json.load(fh)

    unet_files = sorted((n for n in names if n.startswith("unet_")), key=_unet_index)
    imagen_files = [n for n in names if n.startswith("imagen_")]
    if not imagen_files:
        raise IndexError(f"no imagen_*.json under {pdir}")          # generate.py:66 indexes [0] of an empty list
    return [read(n) for n in unet_files], read(imagen_files[0])


def _checkpoint_files(directory: str, ema: bool = False):
    """generate.py:95-119: ``state_dicts/`` (one file per U-Net, ``unet_<i>_state_*.pth``) wins; when it is empty fall back
    to the rolling checkpoints in ``tmp/`` (``unet_<i>_tmp.pth``); both empty is a ValueError.  ``ema=True``: the same rules over
    ``ema_state_dicts/`` and ``ema_tmp/``, the averaged weights a training loop with an EMA writes."""
    best, rolling = ("ema_state_dicts", "ema_tmp") if ema else ("state_dicts", "tmp")
    for sub in (best, rolling):
        folder = os.path.join(directory, sub)
        names = os.listdir(folder) if os.path.isdir(folder) else []
        if ema:
            names = [n for n in names if n.startswith("unet_")]      # (ema_tmp/ also holds the EMA's own state)
        if names:
            if sub == rolling:
                print(f"\n\"{best}\" folder in {directory} is empty, using the most recent checkpoint from \"{rolling}\".\n")
            per_unet = {}
            for n in names:
                if n.startswith("unet_"):
                    per_unet.setdefault(_unet_index(n), n)       # first listing hit per U-Net, as the reference takes [0]
            count = max(per_unet) + 1
            return [os.path.join(folder, per_unet[i]) for i in range(count)]
    if ema:
        raise ValueError(f"Neither \"/ema_state_dicts\" nor \"/ema_tmp\" in {directory} holds a U-Net file. "
                         f"Train with an EMA (MinimagenTrain(..., ema=EMA(imagen))) to acquire averaged state dictionaries. ")
    raise ValueError(f"Both \"/state_dicts\" and \"/tmp\" in {directory} are empty. "
                     f"Train the model to acquire state dictionaries for inference. ")


def load_minimagen(directory: str, ema: bool = False) -> Imagen:
    """generate.py:79-121: instantiate from the parameter files, then load each U-Net's checkpoint.  ``ema=True`` (not in the reference)
    loads the exponentially averaged weights instead; a directory written without an EMA raises ValueError."""
    unets_params, imagen_params = load_params(directory)
    model = Imagen(unets=[Unet(**p) for p in unets_params], **imagen_params)
    where = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    for idx, path in enumerate(_checkpoint_files(directory, ema)):
        model.unets[idx].load_state_dict(torch.load(path, map_location=where))
    # the reference leaves the module where it was built and samples there; this implementation has no CPU sampling path,
    # so the loaded model goes to the device the checkpoints were mapped to
    return model.to(where)


def _prepare_output(save_directory: str) -> str:
    """generate.py:12-30: ``<save_directory>/generated_images`` must be new or empty."""
    root = os.path.abspath(save_directory)
    img_dir = os.path.join(root, "generated_images")
    if not os.path.exists(img_dir):
        os.makedirs(img_dir)
    elif os.listdir(img_dir):
        raise FileExistsError(f"The directory {img_dir} already exists and is nonempty")
    return root


def sample_and_save(captions: list, *, minimagen: Optional[Imagen] = None, training_directory: Optional[str] = None,
                    sample_args: dict = {}, save_directory: Optional[str] = None, filetype: str = "png", ema: bool = False):
    """generate.py:124-173: writes ``captions.txt`` (+ ``imagen_training_directory.txt``) into ``save_directory`` and
    ``generated_images/image_<caption index>.<filetype>``; exactly one of ``minimagen`` / ``training_directory``.
    ``sample_args`` goes to ``Imagen.sample`` as keywords -- ``cond_scale``, and the step-count knobs ``sample_steps`` / ``sampler`` /
    ``sampler_eta`` (e.g. ``dict(cond_scale=3., sample_steps=25, sampler='dpmpp_2m')``) among them, and the pixel inputs ``inpaint_images`` /
    ``inpaint_masks`` / ``start_image`` / ``start_at_stage`` / ``stop_at_stage`` (one row per caption), and the guidance extras ``negative_texts`` (one string, or one per caption) /
    ``negative_text_embeds`` / ``negative_text_masks`` / ``guidance_rescale``, and the guidance over the steps ``guidance_interval`` / ``guidance_schedule``,
    and the starting image ``init_images`` (one row per caption) / ``init_strength``, and how x0 is bounded,
    ``thresholding`` ('dynamic' / 'static' / 'none') / ``thresholding_percentile``.  ``ema=True`` loads the training
    directory's averaged weights (``load_minimagen(..., ema=True)``); it needs ``training_directory``."""
    assert not (minimagen is None and training_directory is None), \
        "Must supply either a training directory or MinImagen instance."
    assert (minimagen is not None) ^ (training_directory is not None), \
        "Cannot supply both a MinImagen instance and a training directory"
    if ema and training_directory is None:
        raise ValueError("ema=True selects the checkpoint files of a training directory; with a MinImagen instance, sample inside "
                         "EMA.average_parameters() instead")
    if save_directory is None:
        save_directory = datetime.now().strftime("generated_images_%Y%m%d_%H%M%S")
    root = _prepare_output(save_directory)
    with open(os.path.join(root, "captions.txt"), "w") as fh:
        fh.writelines(f"{c}\n" for c in captions)
    if training_directory is not None:
        with open(os.path.join(root, "imagen_training_directory.txt"), "w") as fh:
            fh.write(training_directory)
        minimagen = load_minimagen(training_directory, ema=ema)
    images = minimagen.sample(texts=captions, return_pil_images=True, **sample_args)
    for idx, im in enumerate(images):
        im.save(os.path.join(root, "generated_images", f"image_{idx}.{filetype}"))
