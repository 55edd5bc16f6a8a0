"""
oracle/ -- CPU restatement of the mycroft-precise hot path.  TEST INFRASTRUCTURE ONLY.

Only ``tests/``, ``__graft_entry__.smoke()`` and the ``cpu_baseline`` leg of ``bench.py``
may import anything from this package, and there only as the *checker*: nothing under
``mycroft_precise_amd/`` imports it, and the product path fails loudly when the HIP
library is missing instead of falling back to this code.

What is restated, and how firmly each piece is pinned
-----------------------------------------------------
* Streaming glue (``Listener.update_vectors`` / ``update``, ``vectorize``,
  ``add_deltas``, ``buffer_to_audio``, ``ThresholdDecoder``) -- restated from
  ``/root/reference/precise/{network_runner,vectorization,util,threshold_decoder,
  functions,params}.py``.  PINNED: ``oracle/gen_golden.py`` runs the reference's own,
  unmodified ``precise.network_runner.Listener`` / ``ThresholdDecoder`` in the build
  container and commits its outputs under ``tests/golden/``; ``tests/test_oracle.py``
  checks this restatement against those fixtures.
* MFCC arithmetic -- third-party **sonopy 0.1.2** (``requirements.txt:35``), NOT vendored
  in the reference and not installable offline.  ``oracle/sonopy_restated.py`` restates
  its published algorithm.  **PARITY UNPINNED** against real sonopy bits.
* GRU / Dense arithmetic -- third-party **Keras 2.2.4 / TensorFlow 1.13.1**
  (``requirements.txt:11,38``), not vendored, not installable.  ``oracle/keras_gru.py``
  restates ``GRUCell.call`` (implementation 1, reset_after=False, hard_sigmoid) and the
  Dense+sigmoid head.  **PARITY UNPINNED** against real Keras/TF bits.
* The bf16-operand network (``gru_precision='bf16'``; not in the reference) -- ``oracle/bf16_gru.py``
  restates the arithmetic contract of ``csrc/gru_bf16_device.h`` / ``gru_b20_device.h`` (which values
  are rounded to bfloat16, and where) on top of ``keras_gru.py``: with the rounding switched off it IS
  ``keras_gru.predict(dtype=float64)`` (``tests/test_bf16_contract_host.py``).

* The offline tools.  Their restatements live under ``tests/`` and each is PINNED by a fixture that a tool under
  ``tools/`` writes from the reference's own script code, imported behind stub modules and an in-memory ``wavio``
  (``tools/reference_stubs.py``), with this package's ``sonopy_restated`` / ``keras_gru`` in the same seams as above:
    - ``tests/augment_reference.py``      <- ``add_noise.npz``          (``tools/make_add_noise_fixture.py``: ``NoiseData``)
    - ``tests/stats_reference.py``        <- ``stats.npz``              (``tools/make_stats_fixture.py``: ``Stats``, ...)
    - ``tests/generated_reference.py``    <- ``train_generated.npz``    (``tools/make_script_fixtures.py``:
      ``TrainGeneratedScript.vectors_from_fn``: labels, draws, merged audio bits, emitted windows)
    - ``tests/incremental_reference.py``  <- ``train_incremental.npz``  (``TrainIncrementalScript.train_on_audio``:
      confidences, hits, saved int16 rings, retrain points)
    - ``tests/sampled_reference.py``      <- ``train_sampled.npz``      (``TrainScript.load_sample_data``,
      ``TrainSampledScript.choose_new_samples`` / ``write_sampling_metrics``: hash table, index sets, metrics lines)
    - ``host_metric`` / ``host_buckets`` (``tests/test_simulate.py``) <- ``simulate.npz`` (``SimulateScript.run``:
      predictions, per-file and total metrics, the printed report)
  ONLY RESTATED, still: Keras' ``fit`` (what ``retrain`` and a sampling cycle train), the ``fitipy`` file format, and the
  set order behind train_sampled's ``islice`` (any subset of the remaining failures is a legal outcome).

So: the golden fixtures pin *the reference's own code* (everything the reference repo
actually owns on this path) with the restated third-party arithmetic plugged into its
documented seams (``sonopy`` module, ``runner_cls``).
"""
